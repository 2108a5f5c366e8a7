// wave_sink.h -- the device Sink of the byte-oriented decompressors (tiff_lzw.h, gif_lzw.h): the output of one segment or frame written
// by one wave whose lanes all run the decoder on the same bits (tiff_kernels.hip, gif_kernels.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The output through one pointer: LDS or global memory (flat addressing).  Lanes read what other lanes wrote, so a copy begins behind a
// workgroup fence (the block is one wave).
struct WaveSink {
    uint8_t *out;
    uint64_t cap_, n;
    uint32_t lane;
    __device__ uint64_t pos() const { return n; }
    __device__ uint64_t cap() const { return cap_; }
    __device__ __forceinline__ void lit(uint32_t b)
    {
        if (lane == 0) out[n] = (uint8_t)b;
        n++;
    }
    __device__ __forceinline__ void copy(uint64_t from, uint32_t len)
    {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        const uint64_t dist = n - from;
        for (uint32_t base = 0; base < len; base += 64) {
            const uint32_t i = base + lane;
            // (every source byte lies below n: no step of a copy reads what an earlier step of it wrote)
            if (i < len) out[n + i] = out[from + (dist >= len ? i : i % dist)];
        }
        n += len;
    }
    __device__ __forceinline__ void span(const uint8_t *p, uint32_t len)
    {
        for (uint32_t i = lane; i < len; i += 64) out[n + i] = p[i];
        n += len;
    }
    __device__ __forceinline__ void fill(uint8_t b, uint32_t len)
    {
        for (uint32_t i = lane; i < len; i += 64) out[n + i] = b;
        n += len;
    }
};
