// kge_tucker.hip -- the body of TuckER (models/projection.py:259-344) in front of the 1-N head of kge_head.hip.
// For a row with entity e and relation r (d1 = entity width, d2 = relation width, W the shared core [d2, d1, d1]):
//     a   = ent[e] / max(|ent[e]|, 1e-12)  * m0            (input dropout, site 0)
//     M   = sum_k rel[r][k] W[k, :, :]     * m1            (hidden dropout 1, site 1, elementwise on the d1 x d1 matrix)
//     z_j = sum_i a_i M_ij
//     x   = z / max(|z|, 1e-12)            * m2            (hidden dropout 2, site 2)
// M is never stored.  Its tiles are products rel_rows[n, d2] x W[d2, (i, j)] on v_mfma_f32_16x16x4_f32 (operand layout of
// kge_mfma_blocks.h): a workgroup keeps 64 batch rows of rel (four 16-row blocks, LDS, read_blocks<4>) and streams W from memory; the
// accumulators of one (i, 16 j) tile are weighted by a_i m1 and added to the z accumulators in registers while i advances
// (k_tucker_core<0>).  The i range is split over workgroups; the partial z rows are added in split order (k_tucker_finish).
//
// Backward, with dz the gradient at z and G_b = (a_b (x) dz_b) o m1_b generated on the fly:
//     g_W[k,i,j]    += sum_b rel[r_b][k] G_b[i,j]      k_tucker_gw:   rel^T x G on the matrix cores, ONE owner per output tile walking
//                                                                      the batch in row order -- bit-identical run to run
//     g_rel[r_b][k] += sum_ij W[k,i,j] G_b[i,j]        k_tucker_grel: G x W^T on the matrix cores, per-row shares added in row order
//     g_a[b][i]      = sum_j M_ij m1 dz_j              k_tucker_core<1>: the forward's tiles again, contracted over j
//     g_ent[e_b]    += g_a through m0 and the first normalisation (k_tucker_gent), added in row order (k_tucker_scatter)
// No kernel of this file uses atomics: with the head's ordered split-K sums the whole step is bit-identical run to run.
//
// The dropout draw is the shared one (kge_projection.h spells the Philox counters out), with
//     elem    = i (site 0), i * d1 + j (site 1), j (site 2);   row = position in the call's row list (the fused step: h rows, then t rows)
// Four consecutive rows share one Philox call: the accumulator layout of the matrix cores holds four consecutive rows of one column
// per lane, so the forward draws once per lane and 16 x 16 tile.  With train = 0 or p = 0 a site draws nothing (compile-time for site 1).
#include "kge_projection.h"
#include "kge_mfma_blocks.h"

namespace kge {

constexpr int kTkRows = 64;        // batch rows of a workgroup's tile: four 16-row blocks
constexpr int kTkKChunk = 256;     // relation columns staged in LDS at a time (64 KB)
constexpr int kTkGwK = 128;        // core slices (k) per k_tucker_gw workgroup: 8 accumulator blocks per wave
constexpr int kTkGwStride = 132;   // LDS row stride of its rel tile: rows 4 apart land 16 banks apart
constexpr float kTkEps = 1e-12f;   // F.normalize

struct TkRng {
    DropKey key;
    uint32_t thr[3];               // per site; thr == 0 and scale == 1 draw nothing
    float scale[3];
};
struct TkArgs {
    const float *ent, *rel, *W;
    int d1, d2;
    int64_t n;
    TkRng g;
};

__device__ __forceinline__ float tk_row_factor(const TkRng& g, int site, int elem, int64_t row) {   // the row-wise sites 0 and 2
    return drop_row_factor(g.key, site, elem, row, g.thr[site], g.scale[site]);
}

// one wave per row: a = normalize(ent[e]) * m0 -> a_out[n, d1], |ent[e]| -> na_out[n]
__global__ void __launch_bounds__(256) k_tucker_prep(TkArgs a, const int64_t* __restrict__ e, int drop, float* __restrict__ a_out,
                                                     float* __restrict__ na_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.n) return;
    const float* __restrict__ src = a.ent + e[row] * a.d1;
    float ss = 0.0f;
    for (int i = lane; i < a.d1; i += 64) ss += src[i] * src[i];
    const float na = sqrtf(wave_sum_xor(ss));
    const float den = fmaxf(na, kTkEps);
    for (int i = lane; i < a.d1; i += 64) {
        float v = src[i] / den;
        if (drop) v *= tk_row_factor(a.g, 0, i, row);
        a_out[row * a.d1 + i] = v;
    }
    if (lane == 0) na_out[row] = na;
}

// MODE 0 (forward): grid (row tiles, tiles of 64 j, splits of i); wave w owns columns 16 (4 blockIdx.y + w) + l; zpart[split][n][d1].
// MODE 1 (backward, g_a): grid (row tiles, groups of 4 i); wave w owns i = 4 blockIdx.y + w and walks every 16-column tile; out[n][d1].
// wt: the epilogue's weights, a[n, d1] (MODE 0, indexed by i) or dz[n, d1] (MODE 1, indexed by j).
template <int MODE, bool DROP>
__global__ void __launch_bounds__(256) k_tucker_core(TkArgs a, const int64_t* __restrict__ r, const float* __restrict__ wt, int i_per,
                                                     float* __restrict__ out) {
    extern __shared__ float As[];   // [k of the chunk][64]: batch row 16 mb + l of the tile at 4 l + mb (read_blocks<4>)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int d1 = a.d1, d2 = a.d2;
    const int64_t d1d1 = (int64_t)d1 * d1, n = a.n;
    const int64_t row0 = (int64_t)blockIdx.x * kTkRows;
    const int njb = (d1 + 15) / 16;
    int i_lo, i_hi, jb_lo, jb_hi;
    if constexpr (MODE == 0) {
        i_lo = (int)blockIdx.z * i_per;
        i_hi = min(d1, i_lo + i_per);
        jb_lo = (int)blockIdx.y * 4 + wave;
        jb_hi = min(njb, jb_lo + 1);
    } else {
        i_lo = (int)blockIdx.y * 4 + wave;
        i_hi = min(d1, i_lo + 1);
        jb_lo = 0;
        jb_hi = njb;
    }
    f32x4v acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t rowgrp0 = (uint32_t)(row0 >> 2) + (uint32_t)g;   // + 4 mb: the Philox row group of this lane's four rows

    for (int kc = 0; kc < d2; kc += kTkKChunk) {
        const int kn = min(kTkKChunk, d2 - kc), kn4 = (kn + 3) & ~3;
        __syncthreads();
        for (int idx = threadIdx.x; idx < kn4 * kTkRows; idx += 256) {
            const int kl = idx >> 6, rl = idx & 63;
            const int64_t row = row0 + rl;
            float v = 0.0f;
            if (row < n && kl < kn) v = a.rel[r[row] * d2 + kc + kl];
            As[kl * kTkRows + 4 * (rl & 15) + (rl >> 4)] = v;
        }
        __syncthreads();
        for (int i = i_lo; i < i_hi; ++i) {
            for (int jb = jb_lo; jb < jb_hi; ++jb) {
                const int j = 16 * jb + l, jc = min(j, d1 - 1);
                // (clamped addresses: rows of As beyond the chunk are zero, columns beyond d1 are dropped below)
                const float* __restrict__ wp = a.W + (int64_t)i * d1 + jc;
                f32x4v c[4];
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) c[mb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
                for (int s = 0; s < kn4; s += 4) {
                    const int k = min(kc + s + g, d2 - 1);
                    const float b = wp[(int64_t)k * d1d1];
                    float av[4];
                    read_blocks<4>(&As[(s + g) * kTkRows], l, av);
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb) c[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mb], b, c[mb], 0, 0, 0);
                }
                // epilogue: lane holds rows row0 + 16 mb + 4 g + reg of column j
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) {
                    float f[4] = {1.0f, 1.0f, 1.0f, 1.0f};
                    if constexpr (DROP) {
                        const Philox x = drop_draw(a.g.key, 1u, (uint32_t)(i * d1 + jc), rowgrp0 + 4u * mb);
#pragma unroll
                        for (int q = 0; q < 4; ++q) f[q] = x.c[q] >= a.g.thr[1] ? a.g.scale[1] : 0.0f;
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int64_t row = min(row0 + 16 * mb + 4 * g + q, n - 1);
                        float w = wt[row * d1 + (MODE == 0 ? i : jc)];
                        if (MODE == 1 && j >= d1) w = 0.0f;
                        acc[mb][q] += (w * f[q]) * c[mb][q];
                    }
                }
            }
        }
    }
    if constexpr (MODE == 0) {
        const int j = 16 * jb_lo + l;
        if (jb_lo < njb && j < d1) {
            float* __restrict__ dst = out + (int64_t)blockIdx.z * n * d1;
#pragma unroll
            for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int64_t row = row0 + 16 * mb + 4 * g + q;
                    if (row < n) dst[row * d1 + j] = acc[mb][q];
                }
        }
    } else {
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v = acc[mb][q];
#pragma unroll
                for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);   // the 16 columns of the lane group
                const int64_t row = row0 + 16 * mb + 4 * g + q;
                if (l == 0 && i_lo < d1 && row < n) out[row * d1 + i_lo] = v;
            }
    }
}

// one wave per row: z = sum of the partial rows in split order, x = normalize(z) * m2; z and |z| are kept for the backward
__global__ void __launch_bounds__(256) k_tucker_finish(TkArgs a, const float* __restrict__ zpart, int splits, int drop,
                                                       float* __restrict__ x, float* __restrict__ z_out, float* __restrict__ nz_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.n) return;
    float ss = 0.0f;
    for (int j = lane; j < a.d1; j += 64) {
        float z = 0.0f;
        for (int s = 0; s < splits; ++s) z += zpart[((int64_t)s * a.n + row) * a.d1 + j];
        z_out[row * a.d1 + j] = z;
        ss += z * z;
    }
    const float nz = sqrtf(wave_sum_xor(ss));
    const float den = fmaxf(nz, kTkEps);
    for (int j = lane; j < a.d1; j += 64) {
        float v = z_out[row * a.d1 + j] / den;   // (written by this lane above)
        if (drop) v *= tk_row_factor(a.g, 2, j, row);
        x[row * a.d1 + j] = v;
    }
    if (lane == 0) nz_out[row] = nz;
}

// one wave per row: dz = d loss / d z from dx through m2 and the second normalisation
__global__ void __launch_bounds__(256) k_tucker_bwd_prep(TkArgs a, const float* __restrict__ dx, const float* __restrict__ z,
                                                         const float* __restrict__ nz, int drop, float* __restrict__ dz) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.n) return;
    const float norm = nz[row], den = fmaxf(norm, kTkEps);
    float dot = 0.0f;
    for (int j = lane; j < a.d1; j += 64) {
        float g = dx[row * a.d1 + j];
        if (drop) g *= tk_row_factor(a.g, 2, j, row);
        dot += (z[row * a.d1 + j] / den) * g;
    }
    dot = norm >= kTkEps ? wave_sum_xor(dot) : 0.0f;   // below eps the divisor is the constant eps
    for (int j = lane; j < a.d1; j += 64) {
        float g = dx[row * a.d1 + j];
        if (drop) g *= tk_row_factor(a.g, 2, j, row);
        dz[row * a.d1 + j] = (g - (z[row * a.d1 + j] / den) * dot) / den;
    }
}

// one wave per row: g_a through m0 and the first normalisation = the row's share of g_ent[e], written over g_a
__global__ void __launch_bounds__(256) k_tucker_gent(TkArgs a, const int64_t* __restrict__ e, float* __restrict__ ga,
                                                     const float* __restrict__ na, int drop) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.n) return;
    const float* __restrict__ src = a.ent + e[row] * a.d1;
    const float norm = na[row], den = fmaxf(norm, kTkEps);
    float dot = 0.0f;
    for (int i = lane; i < a.d1; i += 64) {
        float g = ga[row * a.d1 + i];
        if (drop) g *= tk_row_factor(a.g, 0, i, row);
        dot += (src[i] / den) * g;
    }
    dot = norm >= kTkEps ? wave_sum_xor(dot) : 0.0f;
    for (int i = lane; i < a.d1; i += 64) {
        float g = ga[row * a.d1 + i];
        if (drop) g *= tk_row_factor(a.g, 0, i, row);
        ga[row * a.d1 + i] = (g - (src[i] / den) * dot) / den;   // (this lane read element i above)
    }
}

// dst[ids[b]] += sum_s part[s][b] for every row b, in row order and without atomics: the wave of the FIRST row that names an id owns
// that id, walks the later rows 64 at a time (ballot) and adds their shares in order -- bit-identical run to run.
__global__ void __launch_bounds__(256) k_tucker_scatter(const int64_t* __restrict__ ids, int64_t n, int width, const float* __restrict__ part,
                                                        int splits, float* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int64_t id = ids[row];
    bool dup = false;
    for (int64_t b = lane; b < row; b += 64) dup |= ids[b] == id;
    if (__any(dup)) return;   // (wave-uniform)
    for (int c0 = 0; c0 < width; c0 += 64) {
        const int c = c0 + lane;
        float sum = 0.0f;
        for (int64_t b0 = row & ~(int64_t)63; b0 < n; b0 += 64) {
            const int64_t b = b0 + lane;
            unsigned long long m = __ballot(b >= row && b < n && ids[b] == id);
            while (m) {
                const int64_t src = b0 + __builtin_ctzll(m);
                m &= m - 1;
                if (c < width)
                    for (int sp = 0; sp < splits; ++sp) sum += part[((int64_t)sp * n + src) * width + c];
            }
        }
        if (c < width) dst[id * width + c] += sum;
    }
}

// g_W[k, i, j] += sum_b rel[r_b][k] G_b[i, j].  grid (ceil(d1 * njb / 4), ceil(d2 / 128)): wave w owns the output tile (i, 16 j) number
// 4 blockIdx.x + w for the 128 core slices k of blockIdx.y and walks ALL batch rows in order, 64 at a time (their rel rows in LDS).
// In the matrix-core product the batch is the contraction: lane group g takes rows 16 q + 4 g + w in step w of a 16-row group, so one
// Philox call (four consecutive rows of one element) serves four steps.
template <bool DROP>
__global__ void __launch_bounds__(256) k_tucker_gw(TkArgs a, const int64_t* __restrict__ r, const float* __restrict__ av,
                                                   const float* __restrict__ dz, float* __restrict__ g_W) {
    __shared__ float Rs[kTkRows * kTkGwStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int d1 = a.d1, d2 = a.d2;
    const int64_t d1d1 = (int64_t)d1 * d1, n = a.n;
    const int njb = (d1 + 15) / 16;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    const bool live = tile < (int64_t)d1 * njb;
    const int i = live ? (int)(tile / njb) : 0, jb = live ? (int)(tile % njb) : 0;
    const int j = 16 * jb + l, jc = min(j, d1 - 1);
    const int k0 = (int)blockIdx.y * kTkGwK;
    const int nkb = min(8, (d2 - k0 + 15) / 16);
    f32x4v acc[8];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) acc[kb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t b0 = 0; b0 < n; b0 += kTkRows) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < kTkRows * kTkGwK; idx += 256) {
            const int bl = idx >> 7, kl = idx & 127;
            float v = 0.0f;
            if (b0 + bl < n && k0 + kl < d2) v = a.rel[r[b0 + bl] * d2 + k0 + kl];
            Rs[bl * kTkGwStride + kl] = v;
        }
        __syncthreads();
        if (!live) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (b0 + 16 * q >= n) break;   // (uniform)
            float G[4];
            float f[4] = {1.0f, 1.0f, 1.0f, 1.0f};
            if constexpr (DROP) {
                const Philox x = drop_draw(a.g.key, 1u, (uint32_t)(i * d1 + jc), (uint32_t)((b0 >> 2) + 4 * q + g));
#pragma unroll
                for (int w = 0; w < 4; ++w) f[w] = x.c[w] >= a.g.thr[1] ? a.g.scale[1] : 0.0f;
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int64_t row = min(b0 + 16 * q + 4 * g + w, n - 1);   // (rows past n: their rel rows in LDS are zero)
                G[w] = (av[row * d1 + i] * dz[row * d1 + jc]) * f[w];
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float* __restrict__ rp = &Rs[(16 * q + 4 * g + w) * kTkGwStride + l];
#pragma unroll
                for (int kb = 0; kb < 8; ++kb)
                    if (kb < nkb) acc[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(rp[16 * kb], G[w], acc[kb], 0, 0, 0);
            }
        }
    }
    if (!live || j >= d1) return;
#pragma unroll
    for (int kb = 0; kb < 8; ++kb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + 16 * kb + 4 * g + q;
            if (kb < nkb && k < d2) g_W[(int64_t)k * d1d1 + (int64_t)i * d1 + j] += acc[kb][q];
        }
}

// relpart[split][b][k] = sum over the split's i and all j of W[k, i, j] G_b[i, j] (k_tucker_scatter adds them into g_rel[r_b]).  grid
// (row tiles, ceil(d2 / 64), splits of i): wave w owns the 16 core slices k = 16 (4 blockIdx.y + w) + l for the tile's 64 rows; G is the
// A operand (row b = l of a block, contraction index j = 4 s + g).
template <bool DROP>
__global__ void __launch_bounds__(256) k_tucker_grel(TkArgs a, const int64_t* __restrict__ r, const float* __restrict__ av,
                                                     const float* __restrict__ dz, int i_per, float* __restrict__ relpart) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l = lane & 15, g = lane >> 4;
    const int d1 = a.d1, d2 = a.d2;
    const int64_t d1d1 = (int64_t)d1 * d1, n = a.n;
    const int64_t row0 = (int64_t)blockIdx.x * kTkRows;
    const int kb = (int)blockIdx.y * 4 + wave;
    if (16 * kb >= d2) return;   // (no barrier in this kernel)
    const int kc = min(16 * kb + l, d2 - 1);
    const int i_lo = (int)blockIdx.z * i_per, i_hi = min(d1, i_lo + i_per);
    int64_t rows[4];
    bool valid[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        valid[mb] = row0 + 16 * mb + l < n;
        rows[mb] = min(row0 + 16 * mb + l, n - 1);
    }
    f32x4v acc[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = i_lo; i < i_hi; ++i) {
        float ai[4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) ai[mb] = valid[mb] ? av[rows[mb] * d1 + i] : 0.0f;
        const float* __restrict__ wp = a.W + (int64_t)kc * d1d1 + (int64_t)i * d1;
        for (int jj = 0; jj < d1; jj += 4) {
            const int j = jj + g, jc = min(j, d1 - 1);
            const float b = j < d1 ? wp[jc] : 0.0f;
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                float G = ai[mb] * dz[rows[mb] * d1 + jc];
                if constexpr (DROP) {
                    const Philox x = drop_draw(a.g.key, 1u, (uint32_t)(i * d1 + jc), (uint32_t)(rows[mb] >> 2));
                    G *= drop_word(x, (int)(rows[mb] & 3)) >= a.g.thr[1] ? a.g.scale[1] : 0.0f;
                }
                acc[mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(G, b, acc[mb], 0, 0, 0);
            }
        }
    }
    const int k = 16 * kb + l;
    if (k >= d2) return;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t row = row0 + 16 * mb + 4 * g + q;
            if (row < n) relpart[((int64_t)blockIdx.z * n + row) * d2 + k] = acc[mb][q];
        }
}

// ------------------------------------------------------------------------------------------------------------------ host side
static int tk_check(const kge_tucker_desc* d, const char* who, bool grads) {
    if (!d) { set_error("%s: null descriptor", who); return -1; }
    if (!d->ent || !d->rel || !d->W) { set_error("%s: null tables (ent, rel and W are all required)", who); return -1; }
    if (d->tot_entity <= 0 || d->tot_relation <= 0 || d->d1 <= 0 || d->d2 <= 0) {
        set_error("%s: tot_entity, tot_relation, d1 and d2 must be positive (got %lld, %lld, %d, %d)", who, (long long)d->tot_entity,
                  (long long)d->tot_relation, d->d1, d->d2);
        return -1;
    }
    if (d->d1 > 32768) { set_error("%s: d1 = %d: a core slice has more than 2^30 elements", who, d->d1); return -1; }
    const float p[3] = {d->input_dropout, d->hidden_dropout1, d->hidden_dropout2};
    if (drop_check(who, p, 3, d->offset)) return -1;
    if (grads && (!d->g_ent || !d->g_rel || !d->g_W)) {
        set_error("%s: null gradient buffers (g_ent, g_rel and g_W are all required)", who);
        return -1;
    }
    return 0;
}

static bool tk_drop(const kge_tucker_desc* d, int site) {
    const float p[3] = {d->input_dropout, d->hidden_dropout1, d->hidden_dropout2};
    return d->train != 0 && p[site] > 0.0f;
}

static TkArgs tk_args(const kge_tucker_desc* d, int64_t n) {
    TkArgs a{};
    a.ent = d->ent; a.rel = d->rel; a.W = d->W;
    a.d1 = d->d1; a.d2 = d->d2; a.n = n;
    a.g.key = drop_key(d->seed, d->offset);
    const float p[3] = {d->input_dropout, d->hidden_dropout1, d->hidden_dropout2};
    for (int s = 0; s < 3; ++s) {
        a.g.thr[s] = drop_thr(p[s]);
        a.g.scale[s] = drop_scale(p[s]);
    }
    return a;
}

static int tk_row_tiles(int64_t n) { return (int)((n + kTkRows - 1) / kTkRows); }
// rows of W handled by one workgroup of the forward (and of k_tucker_grel): enough workgroups to fill the device, a function of the
// shapes alone (the split order is the summation order)
static int tk_i_per(int64_t n, int d1, int col_tiles) {
    const int64_t base = (int64_t)tk_row_tiles(n) * col_tiles;
    int64_t splits = (1024 + base - 1) / base;
    if (splits > d1) splits = d1;
    if (splits < 1) splits = 1;
    return (int)((d1 + splits - 1) / splits);
}
static int tk_splits(int d1, int i_per) { return (d1 + i_per - 1) / i_per; }
static size_t tk_core_lds(int d2) { const int kn4 = ((d2 < kTkKChunk ? d2 : kTkKChunk) + 3) & ~3; return (size_t)kn4 * kTkRows * sizeof(float); }

static size_t tk_fwd_bytes(const kge_tucker_desc* d, int64_t n) {
    const int per = tk_i_per(n, d->d1, (d->d1 + 63) / 64);
    return align256((size_t)tk_splits(d->d1, per) * (size_t)n * d->d1 * sizeof(float));
}
static int tk_rel_i_per(const kge_tucker_desc* d, int64_t n) { return tk_i_per(n, d->d1, (d->d2 + 63) / 64); }
// dz [n, d1] | g_a [n, d1] | relpart [splits, n, d2]
static size_t tk_bwd_bytes(const kge_tucker_desc* d, int64_t n) {
    return 2 * align256((size_t)n * d->d1 * sizeof(float)) +
           align256((size_t)tk_splits(d->d1, tk_rel_i_per(d, n)) * (size_t)n * d->d2 * sizeof(float));
}
static size_t tk_saved_floats(const kge_tucker_desc* d, int64_t n) { return (size_t)n * (2 * (size_t)d->d1 + 2); }

static int tk_forward(const kge_tucker_desc* d, const int64_t* e, const int64_t* r, int64_t n, float* x, float* saved, void* ws,
                      hipStream_t s) {
    const TkArgs a = tk_args(d, n);
    float *av = saved, *z = saved + n * d->d1, *na = z + n * d->d1, *nz = na + n;
    float* zpart = (float*)ws;
    const unsigned row_blocks = (unsigned)((n + 3) / 4);
    hipLaunchKernelGGL(k_tucker_prep, dim3(row_blocks), dim3(256), 0, s, a, e, (int)tk_drop(d, 0), av, na);
    const int per = tk_i_per(n, d->d1, (d->d1 + 63) / 64), splits = tk_splits(d->d1, per);
    const dim3 grid((unsigned)tk_row_tiles(n), (unsigned)((d->d1 + 63) / 64), (unsigned)splits);
    if (tk_drop(d, 1)) hipLaunchKernelGGL((k_tucker_core<0, true>), grid, dim3(256), tk_core_lds(d->d2), s, a, r, av, per, zpart);
    else hipLaunchKernelGGL((k_tucker_core<0, false>), grid, dim3(256), tk_core_lds(d->d2), s, a, r, av, per, zpart);
    if (int rc = check_launch("k_tucker_prep / k_tucker_core<0>")) return rc;
    hipLaunchKernelGGL(k_tucker_finish, dim3(row_blocks), dim3(256), 0, s, a, zpart, splits, (int)tk_drop(d, 2), x, z, nz);
    return check_launch("k_tucker_finish");
}

static int tk_backward(const kge_tucker_desc* d, const int64_t* e, const int64_t* r, int64_t n, const float* dx, const float* saved,
                       void* ws, hipStream_t s) {
    const TkArgs a = tk_args(d, n);
    const float *av = saved, *z = saved + n * d->d1, *na = z + n * d->d1, *nz = na + n;
    float* dz = (float*)ws;
    float* ga = (float*)((char*)ws + align256((size_t)n * d->d1 * sizeof(float)));
    float* relpart = (float*)((char*)ws + 2 * align256((size_t)n * d->d1 * sizeof(float)));
    const unsigned row_blocks = (unsigned)((n + 3) / 4);
    const bool drop1 = tk_drop(d, 1);
    hipLaunchKernelGGL(k_tucker_bwd_prep, dim3(row_blocks), dim3(256), 0, s, a, dx, z, nz, (int)tk_drop(d, 2), dz);
    const int njb = (d->d1 + 15) / 16;
    const dim3 gw_grid((unsigned)(((int64_t)d->d1 * njb + 3) / 4), (unsigned)((d->d2 + kTkGwK - 1) / kTkGwK));
    if (drop1) hipLaunchKernelGGL((k_tucker_gw<true>), gw_grid, dim3(256), 0, s, a, r, av, dz, d->g_W);
    else hipLaunchKernelGGL((k_tucker_gw<false>), gw_grid, dim3(256), 0, s, a, r, av, dz, d->g_W);
    if (int rc = check_launch("k_tucker_bwd_prep / k_tucker_gw")) return rc;
    const int kt = (d->d2 + 63) / 64;
    const int per = tk_rel_i_per(d, n), rel_splits = tk_splits(d->d1, per);
    const dim3 gr_grid((unsigned)tk_row_tiles(n), (unsigned)kt, (unsigned)rel_splits);
    if (drop1) hipLaunchKernelGGL((k_tucker_grel<true>), gr_grid, dim3(256), 0, s, a, r, av, dz, per, relpart);
    else hipLaunchKernelGGL((k_tucker_grel<false>), gr_grid, dim3(256), 0, s, a, r, av, dz, per, relpart);
    hipLaunchKernelGGL(k_tucker_scatter, dim3(row_blocks), dim3(256), 0, s, r, n, d->d2, relpart, rel_splits, d->g_rel);
    const dim3 ga_grid((unsigned)tk_row_tiles(n), (unsigned)((d->d1 + 3) / 4));
    if (drop1) hipLaunchKernelGGL((k_tucker_core<1, true>), ga_grid, dim3(256), tk_core_lds(d->d2), s, a, r, dz, 1, ga);
    else hipLaunchKernelGGL((k_tucker_core<1, false>), ga_grid, dim3(256), tk_core_lds(d->d2), s, a, r, dz, 1, ga);
    if (int rc = check_launch("k_tucker_grel / k_tucker_core<1>")) return rc;
    hipLaunchKernelGGL(k_tucker_gent, dim3(row_blocks), dim3(256), 0, s, a, e, ga, na, (int)tk_drop(d, 0));
    hipLaunchKernelGGL(k_tucker_scatter, dim3(row_blocks), dim3(256), 0, s, e, n, d->d1, ga, 1, d->g_ent);
    return check_launch("k_tucker_gent / k_tucker_scatter");
}

// fused step: ids [4B int64] | x [2B, d1] | dx [2B, d1] | saved | max(forward, backward, head)
struct TkStepPlan {
    size_t ids, x, dx, saved, rest, total;
};
static TkStepPlan tk_step_plan(const kge_tucker_desc* d, int64_t B, int64_t n_hr, int64_t n_tr) {
    TkStepPlan p{};
    const int64_t n = 2 * B;
    const size_t xb = align256((size_t)n * d->d1 * sizeof(float));
    p.ids = 0;
    p.x = align256((size_t)2 * n * sizeof(int64_t));
    p.dx = p.x + xb;
    p.saved = p.dx + xb;
    p.rest = p.saved + align256(tk_saved_floats(d, n) * sizeof(float));
    size_t rest = tk_fwd_bytes(d, n);
    if (tk_bwd_bytes(d, n) > rest) rest = tk_bwd_bytes(d, n);
    const size_t h1 = kge_head_1n_bce_workspace_bytes(B, d->tot_entity, n_hr), h2 = kge_head_1n_bce_workspace_bytes(B, d->tot_entity, n_tr);
    if (h1 > rest) rest = h1;
    if (h2 > rest) rest = h2;
    p.total = p.rest + align256(rest);
    return p;
}

// the rank pass's body (kge_projection.hip): model.eval(), so no dropout; ws = saved | the forward's partial rows
static int tk_eval_body(const void* desc, const int64_t* e, const int64_t* r, int64_t n, float* x, void* ws, size_t, hipStream_t s) {
    kge_tucker_desc ev = *(const kge_tucker_desc*)desc;
    ev.train = 0;
    const size_t saved = align256(tk_saved_floats(&ev, 2 * n) * sizeof(float));
    return tk_forward(&ev, e, r, 2 * n, x, (float*)ws, (char*)ws + saved, s);
}
static ProjectionEval tk_eval(const kge_tucker_desc* d, int64_t n) {
    const int64_t rows = 2 * (n > 0 ? n : 1);
    return ProjectionEval{d->d1, d->tot_entity, d->tot_relation, d->ent,
                          align256(tk_saved_floats(d, rows) * sizeof(float)) + tk_fwd_bytes(d, rows), tk_eval_body};
}

}  // namespace kge

using namespace kge;

extern "C" {

size_t kge_tucker_saved_floats(const kge_tucker_desc* d, int64_t n) {
    return tk_check(d, "kge_tucker_saved_floats", false) || n < 0 ? 0 : tk_saved_floats(d, n);
}

size_t kge_tucker_body_forward_workspace_bytes(const kge_tucker_desc* d, int64_t n) {
    return tk_check(d, "kge_tucker_body_forward_workspace_bytes", false) || n < 0 ? 0 : tk_fwd_bytes(d, n > 0 ? n : 1);
}

int kge_tucker_body_forward(const kge_tucker_desc* d, const int64_t* e, const int64_t* r, int64_t n, float* x, float* saved,
                            void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_tucker_body_forward";
    if (tk_check(d, who, false)) return -1;
    if (n < 0 || (n > 0 && (!e || !r || !x || !saved))) { set_error("%s: bad arguments", who); return -1; }
    if (ws_check(who, workspace, workspace_bytes, tk_fwd_bytes(d, n > 0 ? n : 1))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_er_ids(who, d->tot_entity, d->tot_relation, e, r, n, s)) return rc;
    return tk_forward(d, e, r, n, x, saved, workspace, s);
}

size_t kge_tucker_body_backward_workspace_bytes(const kge_tucker_desc* d, int64_t n) {
    return tk_check(d, "kge_tucker_body_backward_workspace_bytes", false) || n < 0 ? 0 : tk_bwd_bytes(d, n > 0 ? n : 1);
}

int kge_tucker_body_backward(const kge_tucker_desc* d, const int64_t* e, const int64_t* r, int64_t n, const float* dx, const float* saved,
                             void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "kge_tucker_body_backward";
    if (tk_check(d, who, true)) return -1;
    if (n < 0 || (n > 0 && (!e || !r || !dx || !saved))) { set_error("%s: bad arguments", who); return -1; }
    if (ws_check(who, workspace, workspace_bytes, tk_bwd_bytes(d, n > 0 ? n : 1))) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_er_ids(who, d->tot_entity, d->tot_relation, e, r, n, s)) return rc;
    return tk_backward(d, e, r, n, dx, saved, workspace, s);
}

size_t kge_tucker_train_bce_workspace_bytes(const kge_tucker_desc* d, int64_t batch, int64_t n_hr, int64_t n_tr) {
    if (tk_check(d, "kge_tucker_train_bce_workspace_bytes", false) || batch < 0 || n_hr < 0 || n_tr < 0) return 0;
    return tk_step_plan(d, batch > 0 ? batch : 1, n_hr, n_tr).total;
}

int kge_tucker_train_bce(const kge_tucker_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t batch,
                         const int64_t* hr_off, const int32_t* hr_ids, int64_t n_hr, const int64_t* tr_off, const int32_t* tr_ids,
                         int64_t n_tr, float label_smoothing, void* workspace, size_t workspace_bytes, float* loss, void* stream) {
    const char* who = "kge_tucker_train_bce";
    if (tk_check(d, who, true)) return -1;
    if (batch < 0 || n_hr < 0 || n_tr < 0 || !loss || (batch > 0 && (!h || !r || !t || !hr_off || !tr_off)) || (n_hr > 0 && !hr_ids) ||
        (n_tr > 0 && !tr_ids)) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    const TkStepPlan p = tk_step_plan(d, batch > 0 ? batch : 1, n_hr, n_tr);
    if (ws_check(who, workspace, workspace_bytes, p.total)) return -1;
    if (batch == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t B = batch, n = 2 * B;
    char* ws = (char*)workspace;
    int64_t* e = (int64_t*)(ws + p.ids);
    int64_t* rr = e + n;
    float *x = (float*)(ws + p.x), *dx = (float*)(ws + p.dx), *saved = (float*)(ws + p.saved);
    void* rest = ws + p.rest;
    const size_t rest_bytes = p.total - p.rest;
    const size_t idb = (size_t)B * sizeof(int64_t);
    if (hipMemcpyAsync(e, h, idb, hipMemcpyDeviceToDevice, s) != hipSuccess || hipMemcpyAsync(e + B, t, idb, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(rr, r, idb, hipMemcpyDeviceToDevice, s) != hipSuccess || hipMemcpyAsync(rr + B, r, idb, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("%s: copying the row ids failed: %s", who, hipGetErrorString(hipGetLastError()));
        return -2;
    }
    if (int rc = check_er_ids(who, d->tot_entity, d->tot_relation, e, rr, n, s)) return rc;
    if (int rc = tk_forward(d, e, rr, n, x, saved, rest, s)) return rc;
    // pred_tails = forward(h, r) against hr_t, pred_heads = forward(t, r) against tr_h: a mean over B * E each, added (utils/trainer.py:159-172)
    if (int rc = kge_head_1n_bce(x, B, d->d1, d->ent, d->tot_entity, nullptr, hr_off, hr_ids, n_hr, label_smoothing, rest, rest_bytes, loss,
                                 dx, d->g_ent, nullptr, stream)) return rc;
    if (int rc = kge_head_1n_bce(x + B * d->d1, B, d->d1, d->ent, d->tot_entity, nullptr, tr_off, tr_ids, n_tr, label_smoothing, rest,
                                 rest_bytes, loss, dx + B * d->d1, d->g_ent, nullptr, stream)) return rc;
    return tk_backward(d, e, rr, n, dx, saved, rest, s);
}

size_t kge_tucker_eval_ranks_workspace_bytes(const kge_tucker_desc* d, int64_t n) {
    return tk_check(d, "kge_tucker_eval_ranks_workspace_bytes", false) || n < 0 ? 0 : projection_eval_workspace_bytes(tk_eval(d, n), n);
}

int kge_tucker_eval_ranks(const kge_tucker_desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                          const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks,
                          int32_t* ties, void* stream) {
    const char* who = "kge_tucker_eval_ranks";
    if (tk_check(d, who, false)) return -1;
    return projection_eval_ranks(who, tk_eval(d, n), d, triples, n, tail_off, tail_ids, head_off, head_ids, workspace, workspace_bytes, ranks,
                                 ties, stream);
}

}  // extern "C"
