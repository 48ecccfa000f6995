// bgzf_host.cpp — HOST, GPU-free: one member's inflate, the BAM header, what tcmi_bamfile_read parses of a file, the record-chain rule (bgzf_host.h).
#include "bgzf_host.h"

#include <algorithm>

bool tcmi_bgzf_inflate(const uint8_t *in, size_t clen, uint8_t *out, size_t ulen, const uint32_t *crc)
{
    if (ulen == 0) return true;
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<Bytef *>(in);
    zs.avail_in = (uInt)clen;
    zs.next_out = out;
    zs.avail_out = (uInt)ulen;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == ulen;
    inflateEnd(&zs);
    if (!ok) return false;
    return !crc || (uint32_t)crc32(crc32(0L, Z_NULL, 0), out, (uInt)ulen) == *crc;
}

// SAM spec §4.2: magic, l_text, text, n_ref, then per reference l_name, name, l_ref
tcmi_parse_error tcmi_bam_header_parse(tcmi_stream_front *s, tcmi_bam_head *h)
{
    auto need = [s](size_t k) { while (s->n < k) if (!s->more || !s->more(s)) return false; return true; };
    if (!need(12) || std::memcmp(s->p, "BAM\1", 4) != 0) return {TCMI_E_FORMAT, "BAM magic missing", 0};
    const size_t l_text = rd32(s->p + 4);
    if (!need(12 + l_text)) return {TCMI_E_FORMAT, "truncated header text", 8};
    h->text.assign((const char *)s->p + 8, l_text);
    size_t o = 8 + l_text;
    const size_t n_ref = rd32(s->p + o);
    o += 4;
    for (size_t r = 0; r < n_ref; ++r) {
        if (!need(o + 4)) return {TCMI_E_FORMAT, "truncated reference list", o};
        const size_t l_name = rd32(s->p + o);
        o += 4;
        if (!need(o + l_name + 4)) return {TCMI_E_FORMAT, "truncated reference name", o};
        h->ref_name.emplace_back((const char *)s->p + o, l_name ? l_name - 1 : 0);
        o += l_name;
        h->ref_len.push_back((int64_t)rd32(s->p + o));
        o += 4;
    }
    h->first_record = o;
    return {};
}

tcmi_parse_error tcmi_bam_front_blocks(const uint8_t *bytes, size_t n, tcmi_bam_front *f)
{
    return tcmi_bgzf_walk(bytes, n, &f->inflated, [f](const tcmi_bgzf_member &m) {
        BlockDesc b;
        b.cin = m.cin;
        b.clen = (uint32_t)m.clen;
        b.ulen = (uint32_t)m.ulen;
        b.uout = m.uout;
        b.entry = -2;                                           // (-2: the block's first record starts where the device finds it)
        // tokens: one per literal / match (each gives >= 1 byte and takes >= 1 bit), one per <= 8 191 stored bytes (a stored
        // deflate block takes >= 5 bytes)
        b.tok_cap = std::min(b.ulen, 8u * b.clen) + b.clen / 2 + 8;
        b.tok = f->tok_total;
        f->tok_total += (2u * b.tok_cap + 3u) & ~3u;            // (as many again behind them: bgzf_symbols' scratch)
        f->pay_dwords = std::max(f->pay_dwords, (uint32_t)(((b.cin & 3u) * 8u + b.clen * 8u + 31u) / 32u + 6u));
        f->blocks.push_back(b);
    });
}

// the BAM header: leading blocks are inflated on this thread until it is complete
tcmi_parse_error tcmi_bam_front_header(const uint8_t *bytes, tcmi_bam_front *f)
{
    struct Head : tcmi_stream_front { const uint8_t *bytes; const std::vector<BlockDesc> *blocks; std::vector<uint8_t> got; size_t nb; } head = {{nullptr, 0, nullptr}, bytes, &f->blocks, {}, 0};
    head.more = [](tcmi_stream_front *s) {                      // one more leading block
        Head &h = *static_cast<Head *>(s);
        if (h.nb >= h.blocks->size()) return false;
        const BlockDesc &b = (*h.blocks)[h.nb++];
        h.got.resize(h.n + b.ulen);
        h.p = h.got.data();
        if (!tcmi_bgzf_inflate(h.bytes + b.cin, b.clen, h.got.data() + h.n, b.ulen, nullptr)) return false;
        h.n = h.got.size();
        return true;
    };
    const tcmi_parse_error e = tcmi_bam_header_parse(&head, f);
    if (e.code) return e;
    // records start `o` bytes into the stream: in block k at offset o - (inflated bytes of the blocks before it)
    const size_t o = f->first_record;
    size_t before = 0, k = 0;
    for (; k < f->blocks.size(); ++k) {
        if (o < before + f->blocks[k].ulen) break;
        f->blocks[k].entry = -1;                                // header only (or empty)
        before += f->blocks[k].ulen;
    }
    if (k < f->blocks.size()) f->blocks[k].entry = (int32_t)(o - before);
    // what is left of the inflated bytes behind the header are the file's first records: their mean size sizes the one-sync path's arrays
    size_t at = o, cnt = 0;
    while (at + 4 <= head.got.size()) {
        const size_t bs = rd32(head.got.data() + at);
        if (bs < 32 || bs > (1u << 24) || at + 4 + bs > head.got.size()) break;
        at += 4 + bs;
        ++cnt;
    }
    if (cnt >= 16) f->rec_bytes_hint = (uint32_t)((at - o) / cnt);
    return {};
}

tcmi_chain_verdict tcmi_bam_chain_check(const BlockDesc *blocks, size_t nb, size_t nb_own, bool ranged, const uint32_t *stat,
                                        const uint32_t *first, const int32_t *over)
{
    tcmi_chain_verdict v;
    auto refuse = [&v](int code, size_t b, const std::string &what) { v.code = code; v.block = b; v.what = what; return v; };
    const auto num = [](long long x) { return std::to_string(x); };
    for (size_t b = 0; b < nb; ++b)
        if (stat[b] == ST_BAD_STREAM || stat[b] == ST_BAD_LENGTH)
            return refuse(TCMI_E_FORMAT, b, "BGZF block " + num((long long)b) + " failed to inflate (deflate stream or ISIZE damaged)");
    for (size_t b = 0; b < nb; ++b)
        if (stat[b] == ST_BAD_CRC) return refuse(TCMI_E_FORMAT, b, "CRC32 mismatch in BGZF block " + num((long long)b));
    int64_t expect = -1;                                        // offset in the next block at which a record must start
    bool open = ranged;                                         // (a range: wherever its first block found one)
    for (size_t b = 0; b < nb_own; ++b) {
        const BlockDesc &d = blocks[b];
        if (d.entry == -1) continue;                            // header only
        if (open && first[b] != 0xFFFFFFFFu) { expect = first[b]; open = false; if (d.entry < 0) v.range_first = (int64_t)d.uout + first[b]; }
        if (open) continue;
        if (stat[b] == ST_BAD_RECORD)
            return refuse(TCMI_E_FORMAT, b, "alignment record with an impossible block_size in BGZF block " + num((long long)b));
        if (d.entry >= 0) expect = d.entry;
        if (first[b] == 0xFFFFFFFFu) {                          // no record starts in this block: it lies inside one, or is empty
            if (expect < (int64_t)d.ulen)
                return refuse(TCMI_E_UNSUPPORTED, b, "no alignment record found where one must start in BGZF block " + num((long long)b) + ": host reader");
            expect -= d.ulen;
            continue;
        }
        if ((int64_t)first[b] != expect || over[b] < 0)
            return refuse(TCMI_E_UNSUPPORTED, b, "the chain of alignment records does not close at BGZF block " + num((long long)b) + " (found a start at " +
                                                     num(first[b]) + ", expected " + num(expect) + "): host reader");
        expect = over[b];
    }
    if (!open && nb_own > 0) v.range_next = (int64_t)(blocks[nb_own - 1].uout + blocks[nb_own - 1].ulen) + expect;
    if (nb_own < nb) {                                          // the range's last record must end in the block taken along
        if (expect > (int64_t)blocks[nb_own].ulen)
            return refuse(TCMI_E_UNSUPPORTED, nb_own, "a record longer than a BGZF block at the end of a block range: host reader");
        expect = 0;
    }
    if (expect > 0)
        return refuse(TCMI_E_UNSUPPORTED, nb - 1, "the last alignment record runs " + num(expect) + " bytes past the end of the file: host reader");
    return v;
}
