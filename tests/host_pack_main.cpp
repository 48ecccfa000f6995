// host_pack_main.cpp — a program of its own around trueconsense_amd/csrc/host_pack.{h,cpp}, built by tests/test_host_pack.py with
// AddressSanitizer + UBSan and run as a child process (no GPU, no HIP, nothing of it loaded into python).
//
//   host_pack_main IN OUT [--threads N] [--slots N] [--stride N] [--layout SHIFT:LEN,SHIFT:LEN,...] [--project-reads 0|1] [--use-fast 0|1]
//                         [--chunk-stages N] [--stage-cap N]
//
// IN and OUT are dumps: records of {char name[16], uint64 bytes, the bytes}, arrays raw and little-endian.
//   IN    n_batch (int64), then per BAM: n_reads (int64), pos, flag, l_qseq, tid, cigar_off, cigar, seq_off, seq as struct tcmi_reads has them
//   OUT   totals (int64: n_reads, n_piled, alg, max_end, n_dropped, f_reads, f_chunks, f_words, f_events, g_reads, n_rounds, n_cigar, n_seqw),
//         ref_ext, f_lenoff, f_event, f_seq, f_chunk (struct tcmi_fast_chunk), f_covrun, g_pos, g_meta, g_lseq, g_cigar, g_seq, g_round_cig,
//         g_round_seq: what readset.cpp copies to the device, in the sizes it copies
// stdout: "packed", or "refused <code> <text>" (no OUT then).  Exit status 0 either way; 2: a bad command line or dump.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <utility>

#include "../trueconsense_amd/csrc/host_pack.h"

namespace {

struct Array { std::unique_ptr<uint8_t[]> p; size_t bytes = 0; };   // (an allocation of exactly the array's size: a read past its end is the sanitizer's to report)

[[noreturn]] void die(const char *what)
{
    std::fprintf(stderr, "host_pack_main: %s\n", what);
    std::exit(2);
}

void read_dump(const char *path, std::vector<std::pair<std::string, Array>> *out)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) die("cannot open the input dump");
    char name[16];
    uint64_t bytes;
    while (in.read(name, 16)) {
        if (!in.read(reinterpret_cast<char *>(&bytes), 8)) die("cut record");
        Array a;
        a.bytes = (size_t)bytes;
        a.p.reset(new uint8_t[a.bytes]);
        if (bytes && !in.read(reinterpret_cast<char *>(a.p.get()), (std::streamsize)bytes)) die("cut record");
        out->emplace_back(std::string(name, strnlen(name, 16)), std::move(a));
    }
}

void put(std::ofstream &out, const char *name, const void *p, size_t bytes)
{
    char field[16] = {0};
    std::strncpy(field, name, 15);
    const uint64_t n = bytes;
    out.write(field, 16);
    out.write(reinterpret_cast<const char *>(&n), 8);
    if (bytes) out.write(static_cast<const char *>(p), (std::streamsize)bytes);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc < 3) die("usage: host_pack_main IN OUT [options]");
    tcmi_host_pack_opts opt;
    tcmi_layout lay;
    int64_t stride = 0;
    for (int a = 3; a + 1 < argc; a += 2) {
        const std::string k = argv[a];
        const char *v = argv[a + 1];
        if (k == "--threads") opt.host_threads = std::atoi(v);
        else if (k == "--slots") opt.slots = std::atoll(v);
        else if (k == "--stride") stride = std::atoll(v);
        else if (k == "--project-reads") opt.project_reads = std::atoi(v) != 0;
        else if (k == "--use-fast") opt.use_fast = std::atoi(v) != 0;
        else if (k == "--chunk-stages") opt.chunk_stages = std::atoi(v);
        else if (k == "--stage-cap") opt.stage_cap = std::atoi(v);
        else if (k == "--layout") {                          // as tcmi_layout_build fills it: end = shift + slot length, no slot: -1
            for (const char *p = v; *p;) {
                char *e;
                const long long shift = std::strtoll(p, &e, 10);
                if (*e != ':') die("--layout wants SHIFT:LEN,...");
                const long long len = std::strtoll(e + 1, &e, 10);
                lay.shift.push_back(shift);
                lay.end.push_back(shift < 0 ? -1 : shift + len);
                p = *e == ',' ? e + 1 : e;
                if (*e && *e != ',') die("--layout wants SHIFT:LEN,...");
            }
        } else die("unknown option");
    }
    std::vector<std::pair<std::string, Array>> in;
    read_dump(argv[1], &in);
    if (in.empty() || in[0].first != "n_batch" || in[0].second.bytes != 8) die("the dump does not start with n_batch");
    int64_t n_batch;
    std::memcpy(&n_batch, in[0].second.p.get(), 8);
    if (n_batch < 1 || in.size() != 1 + (size_t)n_batch * 9) die("the dump does not hold n_batch x 9 arrays");
    std::vector<tcmi_reads> reads((size_t)n_batch);
    std::vector<const tcmi_reads *> batch;
    for (int64_t b = 0; b < n_batch; ++b) {
        tcmi_reads &r = reads[(size_t)b];
        std::memset(&r, 0, sizeof r);
        static const char *const names[9] = {"n_reads", "pos", "flag", "l_qseq", "tid", "cigar_off", "cigar", "seq_off", "seq"};
        const void *p[9];
        for (int k = 0; k < 9; ++k) {
            const auto &rec = in[1 + (size_t)b * 9 + (size_t)k];
            if (rec.first != names[k]) die("arrays out of order");
            p[k] = rec.second.p.get();
        }
        std::memcpy(&r.n_reads, p[0], 8);
        r.pos = static_cast<const int32_t *>(p[1]);
        r.flag = static_cast<const uint16_t *>(p[2]);
        r.l_qseq = static_cast<const int32_t *>(p[3]);
        r.tid = static_cast<const int32_t *>(p[4]);
        r.cigar_off = static_cast<const uint64_t *>(p[5]);
        r.cigar = static_cast<const uint32_t *>(p[6]);
        r.seq_off = static_cast<const uint64_t *>(p[7]);
        r.seq = static_cast<const uint8_t *>(p[8]);
        batch.push_back(&r);
    }

    tcmi_host_packed P;
    int rc = tcmi_host_select(batch.data(), (int32_t)n_batch, stride, lay, opt, &P);
    if (!rc) {
        tcmi_host_plan_chunks(opt, &P);
        rc = tcmi_host_pack_aligned(opt, &P);
    }
    if (rc) {
        std::printf("refused %d %s\n", rc, P.msg);
        return 0;
    }
    tcmi_host_pack_general(&P);

    std::ofstream out(argv[2], std::ios::binary);
    if (!out) die("cannot open the output dump");
    const int64_t nf = (int64_t)P.fsel.size(), ng = (int64_t)P.gsel.size();
    const int64_t totals[13] = {P.n_reads_in, P.n_piled(), P.alg, P.max_end, P.n_dropped, nf, (int64_t)P.chunks.size(), (int64_t)P.f_words,
                                (int64_t)P.f_event.size(), ng, P.n_rounds, P.g_cig, P.g_seqw};
    put(out, "totals", totals, sizeof totals);
    put(out, "ref_ext", P.ref_ext.data(), P.ref_ext.size() * 8);
    put(out, "f_lenoff", P.f_lenoff.data(), (size_t)nf * 4);
    put(out, "f_event", P.f_event.data(), P.f_event.size() * 4);
    put(out, "f_seq", P.f_seq, P.f_words * 4);
    put(out, "f_chunk", P.chunks.data(), P.chunks.size() * sizeof(tcmi_fast_chunk));
    put(out, "f_covrun", P.f_covrun.data(), P.f_covrun.size() * 4);
    put(out, "g_pos", P.g_pos.data(), (size_t)ng * 4);
    put(out, "g_meta", P.g_meta.data(), (size_t)ng * 4);
    put(out, "g_lseq", P.g_lseq.data(), (size_t)ng * 4);
    put(out, "g_cigar", P.g_cigar.data(), (size_t)P.g_cig * 4);
    put(out, "g_seq", P.g_seq.data(), (size_t)P.g_seqw * 4);
    put(out, "g_round_cig", P.g_round_cig.data(), (size_t)(P.n_rounds + 1) * 8);
    put(out, "g_round_seq", P.g_round_seq.data(), (size_t)(P.n_rounds + 1) * 8);
    out.close();
    if (!out) die("cannot write the output dump");
    std::printf("packed\n");
    return 0;
}
