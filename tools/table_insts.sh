#!/bin/bash
# tools/table_insts.sh [TREE] — static instruction counts of build_table (csrc/bgzf_device.h), the device decoder's Huffman table builder,
# per instantiation as block_header uses it: <5, 9> literal/length, <1, 8> distance, <1, 7> code lengths.  CPU only (hipcc cross-compiles
# for gfx950); a measurement, not a test: it only counts.  TREE: a checkout of this repository (default: this one) — `git worktree add
# /tmp/parent <ref>` and tools/table_insts.sh /tmp/parent gives the figures of another commit, by the same tool.
# Per instantiation a stand-alone kernel is compiled: code lengths from global memory into LDS, build_table, every result (cnt, sym, rs,
# the root table, the verdict) back to global memory so that nothing is dropped; the same kernel without the call is compiled too and
# its instructions are subtracted.  Printed: the total, and what the root table's slots cost per 64 of them — the stretch from the first
# bit reversal (the slots' reversed indices) to the first store of the write-back: the body of the loop, if a branch in it goes back to
# the bit reversal or in front of it, else the unrolled stretch divided by its turns.  s_waitcnt and s_nop count: the wave issues them.
# TABLE_INSTS_KEEP=FILE keeps the assembly.
set -euo pipefail
tree=$(cd "${1:-$(dirname "$0")/..}" && pwd)
src=$tree/trueconsense_amd/csrc
tmp=$(mktemp -d)
trap '[ -n "${TABLE_INSTS_KEEP:-}" ] && cp "$tmp/k.s" "$TABLE_INSTS_KEEP"; rm -rf "$tmp"' EXIT
flags=$(printf 'isa-flags:\n\t@echo --offload-arch=$(ARCH) $(CXXFLAGS) $(EXTRA)\n' | make -s --no-print-directory -C "$src" -f Makefile -f - isa-flags | tail -n 1)
# the builder's signature: with the sorted entries and the 16-word table (ent, ol), or without
if grep -q 'tab_t \*ent, uint32_t \*ol' "$src/bgzf_device.h"; then extra_decl='__shared__ tab_t ent[324]; __shared__ uint32_t ol[16];'; extra_args='ent, ol,'; else extra_decl=''; extra_args=''; fi
cat > "$tmp/k.hip" <<EOF
#include "bgzf_device.h"
namespace {
template <int MAXG, int ROOT, int KIND, bool CALL>
__global__ __launch_bounds__(64) void table_kernel(const uint8_t *lens_in, int n, uint32_t *out)
{
    __shared__ uint8_t lens[320];
    __shared__ uint16_t cnt[16], sym[320];
    __shared__ tab_t tab[1 << ROOT];
    __shared__ uint32_t rs[2];
    $extra_decl
    const int lane = threadIdx.x;
    for (int i = lane; i < 320; i += 64) lens[i] = lens_in[i];
    bool ok = true;
    if (CALL) ok = build_table<MAXG, ROOT>(lens, n, cnt, sym, $extra_args tab, KIND, rs);
    else __syncthreads();
    for (int i = lane; i < (1 << ROOT); i += 64) out[i] = tab[i];
    for (int i = lane; i < 320; i += 64) out[1024 + i] = sym[i];
    if (lane < 16) out[2048 + lane] = cnt[lane];
    if (lane < 2) out[2100 + lane] = rs[lane];
    if (lane == 0) out[2110] = ok;
}
template __global__ void table_kernel<5, 9, K_LITLEN, true>(const uint8_t *, int, uint32_t *);
template __global__ void table_kernel<5, 9, K_LITLEN, false>(const uint8_t *, int, uint32_t *);
template __global__ void table_kernel<1, 8, K_DIST, true>(const uint8_t *, int, uint32_t *);
template __global__ void table_kernel<1, 8, K_DIST, false>(const uint8_t *, int, uint32_t *);
template __global__ void table_kernel<1, 7, K_CODELEN, true>(const uint8_t *, int, uint32_t *);
template __global__ void table_kernel<1, 7, K_CODELEN, false>(const uint8_t *, int, uint32_t *);
}
EOF
( cd "$src" && ${HIPCC:-hipcc} $flags -I"$src" --cuda-device-only -S "$tmp/k.hip" -o "$tmp/k.s" 2> "$tmp/k.err" ) || { cat "$tmp/k.err" >&2; exit 3; }
python3 - "$tmp/k.s" "$tree" <<'EOF'
import re, subprocess, sys
lines = open(sys.argv[1]).read().split("\n")
kernels = {}
for name in [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]:
    i = next(k for k, l in enumerate(lines) if l.startswith(name + ":"))
    body = []                                                   # instructions, and labels as "name:"
    for l in lines[i + 1:]:
        if re.match(r"\.Lfunc_end\d+:", l): break
        l = l.split(";")[0].strip()
        if l and (re.match(r"[.\w$]+:$", l) or not l.startswith(".")): body.append(l)
    d = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout
    m = re.search(r"table_kernel<(\d+), (\d+), (?:\([^)]*\))?(\d+), (true|false)>", d)
    kernels[(int(m.group(1)), int(m.group(2)), m.group(4) == "true")] = body
is_label = lambda l: l.endswith(":")
count = lambda ls: sum(1 for l in ls if not is_label(l))
print("build_table of %s" % sys.argv[2])
for (g, root) in ((5, 9), (1, 8), (1, 7)):
    full, shell = kernels[(g, root, True)], kernels[(g, root, False)]
    turns = (1 << root) // 64
    # the slot stage: from the first bit reversal to the first store to global memory behind it
    first = next(k for k, l in enumerate(full) if l.startswith("v_bfrev_b32"))
    end = next(k for k, l in enumerate(full) if k > first and l.startswith("global_store"))
    # ... a loop, if a branch in it goes back to a label at or in front of the bit reversal: its body runs once per 64 slots
    loop = None
    for k in range(first, end):
        m = re.match(r"s_cbranch_\w+ ([.\w$]+)$", full[k])
        if m and m.group(1) + ":" in full[:first + 1]:
            at = len(full[:first + 1]) - 1 - full[:first + 1][::-1].index(m.group(1) + ":")
            loop = count(full[at:k + 1])
    per64 = loop if loop else count(full[first:end]) / turns
    print("  <%d, %d>: %5d static instructions; the slots: %s, %5.1f instructions per 64 slots (%d x 64 slots)" %
          (g, root, count(full) - count(shell), "a loop of %d" % loop if loop else "%d unrolled" % count(full[first:end]), per64, turns))
EOF
