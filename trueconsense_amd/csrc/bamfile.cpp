// bamfile.cpp — HOST: tcmi_bamfile, a BAM file on its way to the device decoder (bam_device.hip): the file's bytes read into pinned
// memory (kept in a pool), what bgzf_host.cpp parses of them (the BGZF block table, the BAM header), and the bytes' copy into HBM.
// The host never decodes the file: it walks the gzip member headers (18 bytes per block) and inflates the first block(s) far enough
// to parse the BAM header; the compressed bytes (a few MB .. tens of MB) cross PCIe once.
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bamfile.h"
#include "tcmi_internal.h"

namespace {
// pinned file buffers are kept for the next file: hipHostMalloc / hipHostFree cost about as much as reading 8 MB
struct PinnedPool {
    std::mutex mu;
    struct Buf { uint8_t *p; size_t cap; };
    std::vector<Buf> free_;
    uint8_t *take(size_t want, size_t *cap)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t k = 0; k < free_.size(); ++k)
                if (free_[k].cap >= want && free_[k].cap <= 2 * want + (1 << 20)) {
                    uint8_t *p = free_[k].p;
                    *cap = free_[k].cap;
                    free_.erase(free_.begin() + (long)k);
                    return p;
                }
        }
        uint8_t *p = nullptr;
        const size_t c = want + want / 8;
        if (hipHostMalloc((void **)&p, c, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        *cap = c;
        return p;
    }
    void give(uint8_t *p, size_t cap)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (free_.size() < 8) { free_.push_back({p, cap}); return; }
        }
        (void)hipHostFree(p);
    }
};
PinnedPool &pinned_pool() { static PinnedPool *p = new PinnedPool(); return *p; }   // (never destroyed: the HIP runtime may be gone by then)
} // namespace

extern "C" {

int tcmi_bamfile_free(tcmi_bamfile *f)
{
    if (!f) return TCMI_OK;
    if (f->bytes) pinned_pool().give(f->bytes, f->pool_cap);
    if (f->d_bytes) (void)hipFree(f->d_bytes);
    delete f;
    return TCMI_OK;
}

// The file's compressed bytes into HBM, to stay there: tcmi_readset_from_bamfile[_blocks] of this file then starts from device
// memory (no PCIe copy per call) — the form in which a file arrives that a peer GPU, a NIC or a storage engine wrote into HBM,
// and the one bench.py's headline times ("inputs resident in HBM when the timed region starts").
int tcmi_bamfile_to_device(tcmi_ctx *ctx, tcmi_bamfile *f)
{
    if (!ctx || !f) return tcmi_fail(ctx, TCMI_E_ARG, "null argument");
    TCMI_HIP(ctx, hipSetDevice(ctx->device));
    if (f->d_bytes && f->d_device == ctx->device) return TCMI_OK;
    if (f->d_bytes) { (void)hipFree(f->d_bytes); f->d_bytes = nullptr; }
    if (hipMalloc((void **)&f->d_bytes, f->cap) != hipSuccess) {
        (void)hipGetLastError();
        f->d_bytes = nullptr;
        return tcmi_fail(ctx, TCMI_E_NOMEM, "hipMalloc(%zu) for the bytes of %s failed", f->cap, f->path.c_str());
    }
    f->d_device = ctx->device;
    TCMI_HIP(ctx, hipMemcpyAsync(f->d_bytes, f->bytes, f->cap, hipMemcpyHostToDevice, ctx->stream));
    TCMI_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TCMI_OK;
}

const char *tcmi_bamfile_path(const tcmi_bamfile *f) { return f ? f->path.c_str() : ""; }

// Read the file into pinned memory; the block table and the BAM header are bgzf_host.cpp's (tcmi_bam_front_blocks, tcmi_bam_front_header).
int tcmi_bamfile_read(const char *path, tcmi_bamfile **out) { return tcmi_bamfile_read_threads(path, 0, out); }

// read_threads: threads that copy the file in (0 = by size: four for a file of several MB, which takes the latency of one file
// from 1.15 to 0.65 ms; a runner that reads several files at a time passes 1 — its reader threads are parallel already, and more
// threads only take cores from the ones that feed the GPU: 42.9 vs 41.7 M positions/s)
int tcmi_bamfile_read_threads(const char *path, int read_threads, tcmi_bamfile **out)
{
    if (!path || !out) return tcmi_fail(nullptr, TCMI_E_ARG, "null argument");
    *out = nullptr;
    static const bool timing = std::getenv("TCMI_READ_TIMING") != nullptr;
    const auto tt0 = std::chrono::steady_clock::now();
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return tcmi_fail(nullptr, TCMI_E_IO, "cannot open %s", path);
    std::fseek(fp, 0, SEEK_END);
    const long sz = std::ftell(fp);
    std::fseek(fp, 0, SEEK_SET);
    if (sz < 0) { std::fclose(fp); return tcmi_fail(nullptr, TCMI_E_IO, "cannot size %s", path); }
    tcmi_bamfile *f = new tcmi_bamfile();
    f->path = path;
    f->n_bytes = (size_t)sz;
    f->cap = ((size_t)sz + 4096 + 15) & ~(size_t)15;            // slack: the inflate kernel stages its input 1 KiB at a time
    // (+ room for the block table behind the bytes, so that ONE copy takes both to the device: a block is at least 28 bytes, usually ~ 2 KB and more)
    const size_t table_room = std::min<size_t>(((size_t)sz / 28 + 2) * sizeof(BlockDesc), ((size_t)sz / 512 + 64) * sizeof(BlockDesc));
    f->bytes = pinned_pool().take(f->cap + table_room + 1024, &f->pool_cap);
    if (!f->bytes) {
        std::fclose(fp);
        delete f;
        return tcmi_fail(nullptr, TCMI_E_NOMEM, "hipHostMalloc(%zu) for %s failed (is a GPU present?)", (size_t)sz + 4096, path);
    }
    // The file's bytes into the pinned buffer: a page-cache copy runs at ~7 GB/s per thread, which for a file of several MB is
    // most of what this function costs — so a few threads take a quarter each (pread on the same descriptor).
    const auto tt1 = std::chrono::steady_clock::now();
    size_t got = 0;
    {
        const int fd = fileno(fp);
        static const int forced = std::getenv("TCMI_READ_THREADS") ? std::atoi(std::getenv("TCMI_READ_THREADS")) : 0;   // (A/B measurements)
        const int n_thr = forced > 0 ? std::min(forced, 16) : read_threads > 0 ? std::min(read_threads, 16) : sz > (4l << 20) ? 4 : sz > (1l << 20) ? 2 : 1;
        std::vector<size_t> part((size_t)n_thr, 0);
        auto piece = [&](int t) {
            const size_t lo = (size_t)sz * (size_t)t / (size_t)n_thr, hi = (size_t)sz * (size_t)(t + 1) / (size_t)n_thr;
            size_t at = lo;
            while (at < hi) {
                const ssize_t r = pread(fd, f->bytes + at, hi - at, (off_t)at);
                if (r <= 0) break;
                at += (size_t)r;
            }
            part[(size_t)t] = at - lo;
        };
        std::vector<std::thread> thr;
        for (int t = 1; t < n_thr; ++t) thr.emplace_back(piece, t);
        piece(0);
        for (auto &t : thr) t.join();
        for (size_t p : part) got += p;
    }
    const auto tt2 = std::chrono::steady_clock::now();
    std::fclose(fp);
    std::memset(f->bytes + f->n_bytes, 0, f->cap - f->n_bytes);
    auto bail = [&](int code, const char *what, size_t at) {
        tcmi_bamfile_free(f);
        return tcmi_fail(nullptr, code, "%s: %s at byte %zu", path, what, at);
    };
    if (got != (size_t)sz) return bail(TCMI_E_IO, "short read", got);
    // The block table, then the BAM header (bgzf_host.cpp: wherever the bytes lie)
    tcmi_parse_error e = tcmi_bam_front_blocks(f->bytes, f->n_bytes, f);
    if (e.code) return bail(e.code, e.what, e.at);
    const auto tt3 = std::chrono::steady_clock::now();
    e = tcmi_bam_front_header(f->bytes, f);
    if (e.code) return bail(e.code, e.what, e.at);
    if (f->blocks.size() * sizeof(BlockDesc) <= table_room) {   // (else: blocks of < 512 bytes — the table goes by a copy of its own)
        f->desc_at = (f->cap + 255) & ~(size_t)255;
        std::memcpy(f->bytes + f->desc_at, f->blocks.data(), f->blocks.size() * sizeof(BlockDesc));
        f->cap = f->desc_at + ((f->blocks.size() * sizeof(BlockDesc) + 255) & ~(size_t)255);      // what goes to the device: bytes, slack, table
    }
    if (timing) {
        const auto tt4 = std::chrono::steady_clock::now();
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return (long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
        std::fprintf(stderr, "[tcmi] bamfile_read %s: open + pinned buffer %ld us, read %ld us, block table %ld us, header %ld us\n", path, us(tt0, tt1), us(tt1, tt2), us(tt2, tt3), us(tt3, tt4));
    }
    *out = f;
    return TCMI_OK;
}

int tcmi_bamfile_ref(const tcmi_bamfile *f, int32_t i, const char **name, int64_t *len)
{
    if (!f || i < 0 || (size_t)i >= f->ref_name.size()) return tcmi_fail(nullptr, TCMI_E_ARG, "no reference %d in the header", i);
    if (name) *name = f->ref_name[(size_t)i].c_str();
    if (len) *len = f->ref_len[(size_t)i];
    return TCMI_OK;
}

int tcmi_bamfile_info(const tcmi_bamfile *f, int64_t *file_bytes, int64_t *inflated_bytes, int64_t *n_blocks, int32_t *n_ref,
                      const char **ref0_name, int64_t *ref0_len)
{
    if (!f) return tcmi_fail(nullptr, TCMI_E_ARG, "bamfile is NULL");
    if (file_bytes) *file_bytes = (int64_t)f->n_bytes;
    if (inflated_bytes) *inflated_bytes = (int64_t)f->inflated;
    if (n_blocks) *n_blocks = (int64_t)f->blocks.size();
    if (n_ref) *n_ref = (int32_t)f->ref_name.size();
    if (ref0_name) *ref0_name = f->ref_name.empty() ? "" : f->ref_name[0].c_str();
    if (ref0_len) *ref0_len = f->ref_len.empty() ? 0 : f->ref_len[0];
    return TCMI_OK;
}

const char *tcmi_bamfile_text(const tcmi_bamfile *f) { return f ? f->text.c_str() : ""; }

} // extern "C"
