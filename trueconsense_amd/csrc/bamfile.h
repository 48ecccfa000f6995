// bamfile.h — struct tcmi_bamfile: what bamfile.cpp (the file reader) fills and bam_device.hip (the device decoder's drivers) reads.
#pragma once
#include "bgzf_host.h"

struct tcmi_bamfile : tcmi_bam_front {          // a BAM file's bytes in pinned host memory + what the host parsed of it
    uint8_t *bytes = nullptr;                   // hipHostMalloc
    uint8_t *d_bytes = nullptr;                 // the same `cap` bytes in HBM (tcmi_bamfile_to_device), or null
    size_t desc_at = 0;                         // the block table (BlockDesc[]) lies behind the file's bytes, at this offset of `bytes` / `d_bytes` (0: it does not)
    int d_device = -1;
    size_t n_bytes = 0, cap = 0;                // cap: bytes that go to the device (file + zeroed slack)
    size_t pool_cap = 0;                        // bytes of the pinned allocation
    std::string path;
};
