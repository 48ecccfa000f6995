"""The rule the device decoder builds a block's Huffman tables by (csrc/huffman_rule.h; csrc/bgzf_device.h: build_table), without a
GPU: tests/huffman_table_main.cpp holds it — and build_table's steps restated lane by lane — against a bit-by-bit canonical decoder, in
a program of its own, plain and under AddressSanitizer + UBSan.  The cases are the program's: every length vector of 6 symbols with
lengths 0-4 at three root bits, random complete and incomplete codes at 7, 8 and 9 root bits, the edges (single codes, all lengths equal
to the root bits or one more, all 15 lengths, the fixed code, no code) and over-subscribed vectors, of which the verdict is compared."""
import pytest

from tests import host_program

SRC = ["tests/huffman_table_main.cpp"]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_the_rule_against_a_bit_by_bit_decoder(tmp_path, sanitize):
    prog = host_program.build(SRC, tmp_path / "huffman_table_main", sanitize=sanitize)
    r = host_program.run(prog)
    word, codes, over, slots = r.stdout.split()
    assert word == "ok", r.stdout[-2000:]
    # 15 625 vectors in the sweep alone; what is compared slot by slot are the codes that are not over-subscribed
    assert int(codes) + int(over) > 15625 + 3 * 1700 + 3000 and int(codes) > 8000 and int(over) > 8000 and int(slots) > 10 ** 6
