// kge_sampler_device.h -- device-side negative corruption shared by the stand-alone sampler (kge_sampler.hip) and the
// fused sample+score+loss+backward training kernel (kge_score.hip).  See kge_sampler.hip for the semantics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/kge_hip.h"

namespace kge {

constexpr unsigned long long kEmpty = 0xFFFFFFFFFFFFFFFFull;

__host__ __device__ __forceinline__ unsigned long long pack_triple(int64_t h, int64_t r, int64_t t) {
    return ((unsigned long long)(h & 0xFFFFFF) << 40) | ((unsigned long long)(r & 0xFFFF) << 24) |
           (unsigned long long)(t & 0xFFFFFF);
}
__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long x) {  // splitmix64 finaliser
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// membership test, one slot per dependent load (the fused push kernels, which have no registers to spare for a wider one)
__host__ __device__ __forceinline__ bool set_contains(const unsigned long long* __restrict__ slots, unsigned long long mask,
                                                      unsigned long long key) {
    unsigned long long s = mix64(key) & mask;
    for (;;) {
        const unsigned long long v = slots[s];
        if (v == key) return true;
        if (v == kEmpty) return false;
        s = (s + 1) & mask;
    }
}

// The same test over the same table, one ALIGNED group of W slots per dependent round trip (W / 2 16-byte loads in flight together;
// W = 8 is one 64-byte line).  The group is scanned in registers in probe order: slots in front of the home slot are ignored in the
// first group only, the first slot equal to the key answers true, the first empty one false, otherwise the next group (wrapping with
// the mask).  A run of linear probing is contiguous modulo the table size, so this visits the slots set_contains visits, in its
// order, and returns what it returns for every table k_set_insert can produce.  The table is a power of two >= 16 slots and its
// base is 16-byte aligned (an allocation of its own), so an aligned group of W <= 16 slots never leaves it.
constexpr int kProbeMaxW = 16;
template <int W>
__host__ __device__ __forceinline__ bool set_contains_wide(const unsigned long long* __restrict__ slots, unsigned long long mask,
                                                           unsigned long long key) {
    static_assert(W >= 2 && W <= kProbeMaxW && (W & (W - 1)) == 0, "a group is a power of two of slots, at most the smallest table");
    const unsigned long long home = mix64(key) & mask;
    unsigned long long base = home & ~(unsigned long long)(W - 1);
    unsigned live = ~0u << (unsigned)(home - base);   // bit j: slot j of the group takes part in the scan
    for (;;) {
        const ulonglong2* __restrict__ g = reinterpret_cast<const ulonglong2*>(slots + base);
        ulonglong2 v[W / 2];
#pragma unroll
        for (int j = 0; j < W / 2; ++j) v[j] = g[j];   // all loads of the group before any compare
        unsigned hit = 0u, stop = 0u;                  // bit j: slot j holds the key / ends the run (key or empty)
#pragma unroll
        for (int j = 0; j < W / 2; ++j) {
            hit |= (v[j].x == key ? 1u : 0u) << (2 * j) | (v[j].y == key ? 2u : 0u) << (2 * j);
            stop |= (v[j].x == kEmpty ? 1u : 0u) << (2 * j) | (v[j].y == kEmpty ? 2u : 0u) << (2 * j);
        }
        stop = (stop | hit) & live;
        if (stop) return (hit & stop & (0u - stop)) != 0u;   // the first slot in probe order that ends the run
        base = (base + W) & mask;
        live = ~0u;
    }
}

// W = 1: the one-slot probe; otherwise the grouped one
template <int W>
__host__ __device__ __forceinline__ bool set_probe(const unsigned long long* __restrict__ slots, unsigned long long mask,
                                                   unsigned long long key) {
    if constexpr (W == 1) return set_contains(slots, mask, key);
    else return set_contains_wide<W>(slots, mask, key);
}
// group width of the kernels whose sampler is the whole kernel or a rider with registers to spare (k_sample, pull_sample_one).
// Measured on the C1 step at 2 / 4 / 8 / 16 (profiles/r17_sampler_probe.md): 2, 4 and 8 are within 0.15 us of each other with 4 the
// lowest in every round, 16 gives back 0.4 us of the 1.05 us gained.
constexpr int kSamplerProbeW = 4;

struct Philox {
    uint32_t c[4];
};
__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) {
    return (uint32_t)(((unsigned long long)a * b) >> 32);
}
// Philox4x32-10 (Salmon et al., SC'11)
__host__ __device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                         uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = mulhi32(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = mulhi32(M1, c2), lo1 = M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    Philox o;
    o.c[0] = c0; o.c[1] = c1; o.c[2] = c2; o.c[3] = c3;
    return o;
}

// one corrupted triple for negative slot `ctr` of positive (h, r, t): Philox block a = 0, 1, 2, ... per attempt,
// word 0 of block 0 decides head/tail, word 1 of each block is the candidate entity.  W: slots per round trip of the membership test
template <int W = 1>
__device__ __forceinline__ void corrupt_one(int64_t h, int64_t r, int64_t t, int64_t E, const float* __restrict__ bern,
                                            const unsigned long long* __restrict__ slots, unsigned long long mask,
                                            unsigned long long seed, unsigned long long ctr, int64_t& oh, int64_t& ot) {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    Philox x = philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, k0, k1);
    const float u = (float)(x.c[0] >> 8) * (1.0f / 16777216.0f);  // 24-bit uniform in [0,1)
    const float prob = bern ? bern[r] : 0.5f;
    const bool corrupt_tail = u > prob;
    uint32_t attempt = 0;
    int64_t e;
    for (;;) {
        e = (int64_t)(((unsigned long long)x.c[1] * (unsigned long long)E) >> 32);  // uniform in [0,E)
        const unsigned long long key = corrupt_tail ? pack_triple(h, r, e) : pack_triple(e, r, t);
        if (slots == nullptr || !set_probe<W>(slots, mask, key)) break;
        ++attempt;
        x = philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), attempt, 0u, k0, k1);
    }
    oh = corrupt_tail ? h : e;
    ot = corrupt_tail ? e : t;
}

// The classification negative of positive (h, r, t) for slot `ctr` (kge_corrupt_typed): counter, key and side decision as
// corrupt_one; the replacement comes from the relation's list for that side (type_off int64 [2, R + 1]: row 0 = the heads seen with
// r, row 1 = the tails; both index type_ids) and is rejected when it equals the replaced entity or the triple is in the set.  Draw a
// (Philox block a) is typed for a < KGE_TYPED_ATTEMPTS and uniform over [0, E) for the KGE_TYPED_UNIFORM_ATTEMPTS after that; an
// empty list has no typed draws (its uniform draws are blocks 0, 1, ...).  The loop is BOUNDED: the entity, or -1 when every draw
// was rejected.
template <int W = 1>
__host__ __device__ __forceinline__ int64_t corrupt_typed_one(int64_t h, int64_t r, int64_t t, int64_t E, int64_t R,
                                                              const float* __restrict__ bern, const int64_t* __restrict__ type_off,
                                                              const int32_t* __restrict__ type_ids,
                                                              const unsigned long long* __restrict__ slots, unsigned long long mask,
                                                              unsigned long long seed, unsigned long long ctr, bool& corrupt_tail) {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    Philox x = philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, k0, k1);
    const float u = (float)(x.c[0] >> 8) * (1.0f / 16777216.0f);
    const float prob = bern ? bern[r] : 0.5f;
    corrupt_tail = u > prob;
    const int64_t* off = type_off + (corrupt_tail ? R + 1 : 0);
    const int64_t lo = off[r], len = off[r + 1] - lo;
    const int64_t replaced = corrupt_tail ? t : h;
    const uint32_t typed = len > 0 ? (uint32_t)KGE_TYPED_ATTEMPTS : 0u, total = typed + (uint32_t)KGE_TYPED_UNIFORM_ATTEMPTS;
    for (uint32_t a = 0;;) {
        const int64_t e = a < typed ? (int64_t)type_ids[lo + (int64_t)(((unsigned long long)x.c[1] * (unsigned long long)len) >> 32)]
                                    : (int64_t)(((unsigned long long)x.c[1] * (unsigned long long)E) >> 32);
        if (e != replaced) {
            const unsigned long long key = corrupt_tail ? pack_triple(h, r, e) : pack_triple(e, r, t);
            if (slots == nullptr || !set_probe<W>(slots, mask, key)) return e;
        }
        if (++a >= total) return -1;
        x = philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), a, 0u, k0, k1);
    }
}


}  // namespace kge
