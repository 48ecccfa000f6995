// bgzf_host.h — HOST, GPU-free: what both readers (bam_reader.cpp: tcmi_bam_load; bamfile.cpp: tcmi_bamfile_read) make of a BAM
// file's container format before any record is decoded — the walk over the BGZF members (RFC 1952 + the BC extra subfield, SAM
// spec §4.1), one member's raw inflate, the BAM header (§4.2) — and the record-chain rule of the device decoder's several-kernel
// path (bam_device.hip: decode_on_device), as a function over the arrays that come back from the device.
//
// Every byte these functions look at comes from the file: untrusted.  Nothing here includes a HIP header or tcmi_internal.h, so a
// plain C++ compiler builds this file and bgzf_host.cpp into a program of its own (tests/bgzf_host_main.cpp, under ASan + UBSan).
// Failures come back as {code, what, byte offset}; the caller words them ("<path>: <what> at byte <n>").
#pragma once
#include <zlib.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tcmi.h"

namespace {
inline uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
} // namespace

// a BGZF block as the device decoder takes it (bgzf_device.h: the kernels read this table)
struct BlockDesc {
    uint64_t cin;        // first byte of the deflate payload in the file
    uint64_t uout;       // first byte of its output in the inflated stream
    uint32_t clen;       // payload bytes
    uint32_t ulen;       // ISIZE
    int32_t entry;       // offset of the first record start inside this block (>= 0), -1: no record walk (header blocks), -2: the block finds it itself
    uint32_t tok_cap;    // tokens this block may produce at most (bgzf_symbols)
    uint64_t tok;        // its first token in the token array
};

// status word of a block (the device decoder's verdict)
enum { ST_OK = 0, ST_BAD_STREAM = 1, ST_BAD_LENGTH = 2, ST_BAD_RECORD = 3, ST_BAD_CRC = 4 };

struct tcmi_parse_error { int code = TCMI_OK; const char *what = ""; size_t at = 0; };        // (code TCMI_OK: none)

struct tcmi_bgzf_member { size_t cin, clen, ulen, uout; uint32_t crc; };      // payload place and size, ISIZE, place in the inflated stream, the trailer's CRC-32

// The members of bytes[0, n), in order, each handed to visit(const tcmi_bgzf_member &); *inflated = the sum of their ISIZEs.
template <class Visit> inline tcmi_parse_error tcmi_bgzf_walk(const uint8_t *bytes, size_t n, size_t *inflated, Visit &&visit)
{
    static const bool prefetch_ahead = std::getenv("TCMI_NO_HEADER_PREFETCH") == nullptr;
    size_t off = 0, uout = 0;
    while (off < n) {
        if (n - off < 18) return {TCMI_E_FORMAT, "truncated BGZF block header", off};
        const uint8_t *h = bytes + off;
        if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return {TCMI_E_FORMAT, "not a BGZF block (is the file a BAM?)", off};
        const size_t xlen = rd16(h + 10);
        if (n - off < 12 + xlen) return {TCMI_E_FORMAT, "truncated BGZF extra field", off};
        size_t bsize = 0;
        for (size_t x = 0; x + 4 <= xlen;) {
            const uint8_t *s = h + 12 + x;
            const size_t slen = rd16(s + 2);
            if (s[0] == 'B' && s[1] == 'C' && slen == 2 && x + 6 <= xlen) bsize = (size_t)rd16(s + 4) + 1;
            x += 4 + slen;
        }
        if (bsize < 12 + xlen + 8 || n - off < bsize) return {TCMI_E_FORMAT, "bad BGZF block size", off};
        // (the chain of headers is a chain of cache misses once other threads have copied the file in — each header lies in some
        //  other core's cache or in memory: ask for the lines where the block after next will probably start; blocks of one file
        //  are of similar size)
        if (prefetch_ahead) {
            const size_t guess = off + 3 * bsize;
            if (guess + 512 < n && guess > 512)
                for (size_t x = guess - 384; x < guess + 384; x += 64) __builtin_prefetch(bytes + x, 0, 1);
        }
        tcmi_bgzf_member m;
        m.cin = off + 12 + xlen;
        m.clen = bsize - 12 - xlen - 8;
        m.crc = rd32(h + bsize - 8);
        m.ulen = rd32(h + bsize - 4);
        m.uout = uout;
        if (m.ulen > 65536) return {TCMI_E_FORMAT, "BGZF block inflates to more than 64 KiB", off};
        visit(m);
        uout += m.ulen;                                         // the blocks' outputs follow each other without gaps: the stream as it inflates
        off += bsize;
    }
    *inflated = uout;
    return {};
}

// One member's raw inflate: clen payload bytes -> exactly ulen bytes at out; crc: the trailer's CRC-32 to hold the bytes against, or
// null (unchecked).  An empty member (ulen 0) passes as it is.
bool tcmi_bgzf_inflate(const uint8_t *in, size_t clen, uint8_t *out, size_t ulen, const uint32_t *crc);

struct tcmi_bam_head {
    std::string text;                           // SAM header text
    std::vector<std::string> ref_name;
    std::vector<int64_t> ref_len;
    size_t first_record = 0;                    // offset of the first alignment record in the inflated stream
};
// The BAM header from the front of the inflated stream, as far as its reader has it: n bytes at p; more(): make more of the
// stream available (p may move: a reader that inflates on demand grows its buffer) — false, or no function: there is no more.
struct tcmi_stream_front { const uint8_t *p; size_t n; bool (*more)(tcmi_stream_front *); };
tcmi_parse_error tcmi_bam_header_parse(tcmi_stream_front *s, tcmi_bam_head *h);

// What the host parses of a file for the device decoder: the block table with every block's token accounting, and the header — for
// which only as many leading blocks are inflated (on this thread, CRC unchecked: the device checks every block's) as it occupies.
struct tcmi_bam_front : tcmi_bam_head {
    std::vector<BlockDesc> blocks;              // entry: -1 header only (or empty), >= 0 the first record, -2 the device finds it
    size_t inflated = 0;                        // bytes of the stream
    size_t tok_total = 0;                       // tokens reserved for all blocks (bgzf_symbols -> bgzf_copy)
    uint32_t pay_dwords = 0;                    // the largest block's payload in dwords + slack (bgzf_symbols' dynamic LDS)
    uint32_t rec_bytes_hint = 0;                // mean bytes of the alignment records behind the header in the blocks inflated for it (0: too few seen)
};
// Two steps, in this order: the block table of bytes[0, n), then the header (and with it the blocks' entry marks and the hint).
tcmi_parse_error tcmi_bam_front_blocks(const uint8_t *bytes, size_t n, tcmi_bam_front *f);
tcmi_parse_error tcmi_bam_front_header(const uint8_t *bytes, tcmi_bam_front *f);

// The record chain of a device decode.  Every block found the first record start in its own bytes by itself — where the header says
// (the first record), or the first offset at which a plausible record starts (htslib cuts its blocks on record boundaries: offset 0;
// other writers fill them to the brim) — and followed the chain of block_size fields from there.  In block order: if every
// block's find is where its predecessor's last record ends, all of them are record starts, by induction from the header.
// blocks[0, nb): the decoded blocks, of which [0, nb_own) are the caller's (a range that does not end with the file has one block
// more: its last record may run into it); stat / first / over: the device's words per block (ST_*; offset of the first record start
// found, 0xFFFFFFFF: none; bytes by which the last record runs into the next blocks, < 0: its size could not be read).
struct tcmi_chain_verdict {
    int code = TCMI_OK;
    size_t block = 0;                           // the offending block (code != TCMI_OK)
    std::string what;
    int64_t range_first = -1, range_next = -1;  // a range's anchors in its own stream: its first record start (where the header does not say), where the next range's first record starts
};
tcmi_chain_verdict tcmi_bam_chain_check(const BlockDesc *blocks, size_t nb, size_t nb_own, bool ranged, const uint32_t *stat,
                                        const uint32_t *first, const int32_t *over);
