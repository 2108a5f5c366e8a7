// blake3.h -- the BLAKE3 compression function (published specification, 32-byte output), shared by the device kernels of
// blake3_kernels.hip and the host-scalar entry rph_blake3_host: one statement of the arithmetic for both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RPH_B3_HD __host__ __device__ __forceinline__

constexpr uint32_t B3_CHUNK_START = 1, B3_CHUNK_END = 2, B3_PARENT = 4, B3_ROOT = 8, B3_KEYED_HASH = 16;
constexpr uint32_t B3_BLOCK_LEN = 64, B3_CHUNK_LEN = 1024;

RPH_B3_HD uint32_t b3_iv(int i)
{
    const uint32_t iv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
    return iv[i];
}

RPH_B3_HD uint32_t b3_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }  // v_alignbit_b32 / v_perm_b32 on the device

RPH_B3_HD void b3_g(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, uint32_t mx, uint32_t my)
{
    a = a + b + mx;
    d = b3_rotr(d ^ a, 16);
    c = c + d;
    b = b3_rotr(b ^ c, 12);
    a = a + b + my;
    d = b3_rotr(d ^ a, 8);
    c = c + d;
    b = b3_rotr(b ^ c, 7);
}

// Message word of round r at position i: the permutation [2,6,3,10,7,0,4,13,1,11,12,5,9,14,15,8] applied r times.  Every index
// is a compile-time constant once the rounds are unrolled, so the permutation is register renaming.
RPH_B3_HD constexpr int b3_sched(int r, int i)
{
    constexpr int P[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
    int k = i;
    for (int j = 0; j < r; j++) k = P[k];
    return k;
}

// compress(cv, block, counter, block_len, flags) truncated to the 8-word chaining value (all that a 32-byte output needs)
RPH_B3_HD void b3_compress(const uint32_t cv[8], const uint32_t m[16], uint64_t counter, uint32_t block_len, uint32_t flags, uint32_t out[8])
{
    uint32_t v0 = cv[0], v1 = cv[1], v2 = cv[2], v3 = cv[3], v4 = cv[4], v5 = cv[5], v6 = cv[6], v7 = cv[7];
    uint32_t v8 = b3_iv(0), v9 = b3_iv(1), v10 = b3_iv(2), v11 = b3_iv(3);
    uint32_t v12 = (uint32_t)counter, v13 = (uint32_t)(counter >> 32), v14 = block_len, v15 = flags;
#define RPH_B3_ROUND(r)                                                              \
    b3_g(v0, v4, v8, v12, m[b3_sched(r, 0)], m[b3_sched(r, 1)]);                   \
    b3_g(v1, v5, v9, v13, m[b3_sched(r, 2)], m[b3_sched(r, 3)]);                   \
    b3_g(v2, v6, v10, v14, m[b3_sched(r, 4)], m[b3_sched(r, 5)]);                  \
    b3_g(v3, v7, v11, v15, m[b3_sched(r, 6)], m[b3_sched(r, 7)]);                  \
    b3_g(v0, v5, v10, v15, m[b3_sched(r, 8)], m[b3_sched(r, 9)]);                  \
    b3_g(v1, v6, v11, v12, m[b3_sched(r, 10)], m[b3_sched(r, 11)]);                \
    b3_g(v2, v7, v8, v13, m[b3_sched(r, 12)], m[b3_sched(r, 13)]);                 \
    b3_g(v3, v4, v9, v14, m[b3_sched(r, 14)], m[b3_sched(r, 15)]);
    RPH_B3_ROUND(0) RPH_B3_ROUND(1) RPH_B3_ROUND(2) RPH_B3_ROUND(3) RPH_B3_ROUND(4) RPH_B3_ROUND(5) RPH_B3_ROUND(6)
#undef RPH_B3_ROUND
    out[0] = v0 ^ v8, out[1] = v1 ^ v9, out[2] = v2 ^ v10, out[3] = v3 ^ v11;
    out[4] = v4 ^ v12, out[5] = v5 ^ v13, out[6] = v6 ^ v14, out[7] = v7 ^ v15;
}

// parent node of two chaining values (counter 0, 64 bytes)
RPH_B3_HD void b3_parent(const uint32_t key[8], const uint32_t l[8], const uint32_t r[8], uint32_t flags, uint32_t out[8])
{
    uint32_t m[16];
    for (int i = 0; i < 8; i++) m[i] = l[i], m[8 + i] = r[i];
    b3_compress(key, m, 0, B3_BLOCK_LEN, flags | B3_PARENT, out);
}
