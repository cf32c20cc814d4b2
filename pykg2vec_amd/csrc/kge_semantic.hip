// kge_semantic.hip -- SLM and SME / SME_BL (pykg2vec/models/pairwise.py:473-724): score, fused hinge step, filtered rank.
//
//   SLM     energy = - r^ . tanh(h^ M1 + t^ M2)                       M1, M2 [d_e, d_r] (contract over their ROWS)
//   SME     gu = mu1 h^ + mu2 r^ + bu,  gv = mv1 t^ + mv2 r^ + bv,     energy = - gu . gv
//   SME_BL  gu = (mu1 h^) * (mu2 r^) + bu,  gv = (mv1 t^) * (mv2 r^) + bv,  energy = + gu . gv   (the reference's sign)
// with x^ = F.normalize(x) and the shared [d, d] matrices applied as M @ x (contract over their COLUMNS).
//
// Train step (the NTN pair route: forward over [positives | negatives] as one batch of 2n, k_hinge_coeffs, backward):
//   k_sem_forward   a workgroup takes 64 triples, lane = triple.  Waves 0-2 normalise h / r / t into LDS (k-major, stride
//                   65: conflict-free for the lane-per-triple reads and for the transposed scatter below); then each of the
//                   four waves runs one of the four [64, d] x [d, d] products (SLM: a half of one of its two [64, d_e] x
//                   [d_e, d_r] products), register-blocked 8 outputs wide.  The products go to the workspace (SoA:
//                   [slot][k][2n], coalesced over the triples), wave 0 fuses the epilogue (SME sums, SME_BL products,
//                   SLM tanh + r^ dot) into the energy.
//   k_sem_backward  per triple: the hidden-layer gradients (written over the products), the transposed products M^T dX,
//                   the normalisation backward, and the entity / relation rows scattered with float atomics.
//   k_sem_wgrad     the shared-matrix (and bias) gradients sum_i L_i (x) R_i as a GEMM over the batch: a fixed split of
//                   the batch into at most kChunks chunks, one [rows, cols] partial per (matrix, chunk) with plain stores,
//   k_sem_wreduce   summed in chunk order -- the mu1 ... bv and M1 / M2 gradients are bit-identical run to run.
// VALU, not MFMA: the weight operand of a product is the same for all 64 triples of a wave, so it is a scalar-cache load
// (s_load, SGPR operand of v_fma) and every multiply-add is one VALU issue with an LDS read amortised over 8 outputs.  The
// f32 MFMA (v_mfma_f32_32x32x2_f32) runs at the same FP32 vector rate on gfx950, so it buys no flops; it would need the
// [d, d] weights staged through LDS (40 KB per matrix at d = 100, on top of the 3 input tiles) and d = 50 padded to 64.
// At the SME preset (d = 50, 100 000 triples) the four products are ~1 GFLOP per step: microseconds at the vector rate.
//
// Filtered rank:
//   SME / SME_BL: with the query side fixed the energy is linear in the candidate's normalised row,
//                 energy(e) = c + q . e^, so k_sem_queries contracts every (h, r, ?) / (?, r, t) into [q | c] and the sweep
//                 is the negated-dot pipeline of kge_eval.hip (pseudo-model KGE_DOT_INTERNAL) over candidate rows [e^ | 1]
//                 (k_sem_cand): k_eval_gemm at >= 512 queries, the VALU sweep below that; ranks, ties, filter counts and
//                 the returned energies all come from that pipeline's one arithmetic.  Nothing [queries, E]-sized.
//   SLM:          NTN's pre-contracted sweep without its bilinear GEMM: P1 = E^ M1, P2 = E^ M2 ([E, d_r], once per
//                 evaluation, stored d_r-major so the sweep reads them coalesced), energy(e) = - sum_j r^_j
//                 tanh(a_j + P2[e][j]) (tail; a = h^ M1) or - sum_j r^_j tanh(P1[e][j] + b_j) (head; b = t^ M2).  Chunks
//                 of 256 test triples are scored into [512, E] and ranked from those rows (ties not counted: -1, as NTN).
#include "kge_internal.h"

namespace kge {

constexpr int kSemTile = 64;     // triples per workgroup: lane = triple
constexpr int kSemLd = 65;       // LDS stride of a k-major tile row
constexpr int kSemOB = 8;        // outputs per register block of a product
constexpr int kSemMaxDim = 100;  // forward 3, backward 6 input-sized tiles in LDS: 6 * 100 * 65 * 4 B = 156 KB
constexpr int kChunks = 128;     // partial slots of the shared-matrix gradients
constexpr int kSub = 32;         // triples per LDS stage of k_sem_wgrad
constexpr int kSlmChunk = 256;   // SLM eval: test triples per scored chunk

static bool is_sme(int model) { return model == KGE_SME || model == KGE_SME_BL; }

// ---------------------------------------------------------------- shapes and workspace
struct SemShape {
    int de, dr;      // entity / relation row widths
    int sw, nslot;   // product slot width and count per triple (SME: A B C D dgu dgv, width d; SLM: U1 U2, width d_r)
    int ntask;       // weight-gradient tasks
    int64_t wsize;   // floats of all shared-matrix (and bias) gradients
};

static SemShape sem_shape(const kge_model_desc* m) {
    SemShape s;
    s.de = m->dim;
    if (is_sme(m->model)) {
        s.dr = m->dim; s.sw = m->dim; s.nslot = 6; s.ntask = 6;
        s.wsize = 4 * (int64_t)m->dim * m->dim + 2 * (int64_t)m->dim;
    } else {
        s.dr = m->rel_dim; s.sw = m->rel_dim; s.nslot = 2; s.ntask = 2;
        s.wsize = 2 * (int64_t)m->dim * m->rel_dim;
    }
    return s;
}

struct SemWs { float *inv, *prod, *part; size_t bytes; };

static SemWs sem_carve(const SemShape& s, int64_t N2, void* ws) {
    SemWs w;
    size_t off = 0;
    char* base = (char*)ws;
    auto take = [&](size_t b) { float* p = base ? (float*)(base + off) : nullptr; off += align256(b); return p; };
    w.inv = take((size_t)3 * N2 * sizeof(float));
    w.prod = take((size_t)s.nslot * s.sw * N2 * sizeof(float));
    w.part = take((size_t)kChunks * s.wsize * sizeof(float));
    w.bytes = off;
    return w;
}

size_t semantic_workspace_bytes(const kge_model_desc* m, int64_t n) { return sem_carve(sem_shape(m), n, nullptr).bytes; }

static int sem_check(const kge_model_desc* m, const char* who) {
    if (m->dim > kSemMaxDim || m->rel_dim > kSemMaxDim || m->rel_dim <= 0) {
        set_error("%s: SLM / SME / SME_BL take hidden sizes 1..%d (got %d / %d)", who, kSemMaxDim, m->dim, m->rel_dim);
        return -1;
    }
    if (is_sme(m->model) && m->rel_dim != m->dim) {
        set_error("%s: SME needs rel_dim == dim (one hidden_size)", who);
        return -1;
    }
    return 0;
}

// ---------------------------------------------------------------- device side
struct SemArgs {
    const float* ent; const float* rel;
    const float* W[4];        // SME: mu1 mu2 mv1 mv2;  SLM: M1 M2 (W[2], W[3] unused)
    const float* bu; const float* bv;
    IdSplit h, r, t;
    int64_t N2;
    int de, dr, sw;
    float* inv; float* prod;
};

// x^ tiles in LDS: region 0 = h (de rows), 1 = r (dr rows), 2 = t (de rows); element k of lane at [k * kSemLd + lane]
__device__ __forceinline__ int sem_region_off(int s, int de, int dr) { return s == 0 ? 0 : s == 1 ? de * kSemLd : (de + dr) * kSemLd; }
__device__ __forceinline__ int sem_tiles_floats(int de, int dr) { return (2 * de + dr) * kSemLd; }

// waves 0..2 normalise input s of the tile's triples into LDS; inverse norms from `inv_in` (backward) or computed (forward)
__device__ __forceinline__ void sem_load_inputs(const SemArgs& a, float* X, int64_t i, bool valid, int wave, int lane,
                                                bool compute) {
    if (wave >= 3) return;
    const int w = wave == 1 ? a.dr : a.de;
    float* dst = X + sem_region_off(wave, a.de, a.dr) + lane;
    if (!valid) {
        for (int c = 0; c < w; ++c) dst[c * kSemLd] = 0.f;
        return;
    }
    const int64_t id = wave == 0 ? a.h.at(i) : wave == 1 ? a.r.at(i) : a.t.at(i);
    const float* row = (wave == 1 ? a.rel : a.ent) + id * w;
    float inv;
    if (compute) {
        float n2 = 0.f;
        for (int c = 0; c < w; ++c) n2 = fmaf(row[c], row[c], n2);
        inv = 1.0f / fmaxf(sqrtf(n2), kEpsNormalize);
        a.inv[wave * a.N2 + i] = inv;
    } else {
        inv = a.inv[wave * a.N2 + i];
    }
    for (int c = 0; c < w; ++c) dst[c * kSemLd] = row[c] * inv;
}

// the four forward products of wave `wave`: input region, weight, product slot, output range, weight strides (o, c)
struct SemTask { int in, slot, olo, ohi, din, so, sc; const float* W; };

template <int MODEL>
__device__ __forceinline__ SemTask sem_fwd_task(const SemArgs& a, int wave) {
    SemTask k;
    if constexpr (MODEL == KGE_SLM) {   // x @ M: element (o, c) = M[c][o]; half of the outputs per wave
        const int half = (a.dr + 1) / 2;
        k.in = wave < 2 ? 0 : 2; k.slot = wave < 2 ? 0 : 1; k.W = wave < 2 ? a.W[0] : a.W[1];
        k.olo = (wave & 1) ? half : 0; k.ohi = (wave & 1) ? a.dr : half;
        k.din = a.de; k.so = 1; k.sc = a.dr;
    } else {                            // M @ x: element (o, c) = M[o][c]
        k.in = wave == 0 ? 0 : wave == 2 ? 2 : 1; k.slot = wave; k.W = a.W[wave];
        k.olo = 0; k.ohi = a.de; k.din = a.de; k.so = a.de; k.sc = 1;
    }
    return k;
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_sem_forward(SemArgs a, float* __restrict__ scores) {
    extern __shared__ float X[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t i = (int64_t)blockIdx.x * kSemTile + lane;
    const bool valid = i < a.N2;
    sem_load_inputs(a, X, i, valid, wave, lane, true);
    __syncthreads();
    const SemTask k = sem_fwd_task<MODEL>(a, wave);
    const float* xin = X + sem_region_off(k.in, a.de, a.dr) + lane;
    for (int o0 = k.olo; o0 < k.ohi; o0 += kSemOB) {
        float acc[kSemOB];
#pragma unroll
        for (int j = 0; j < kSemOB; ++j) acc[j] = 0.f;
        for (int c = 0; c < k.din; ++c) {
            const float x = xin[c * kSemLd];
#pragma unroll
            for (int j = 0; j < kSemOB; ++j) {
                const int o = min(o0 + j, k.ohi - 1);
                acc[j] = fmaf(k.W[(int64_t)o * k.so + (int64_t)c * k.sc], x, acc[j]);
            }
        }
        if (valid)
#pragma unroll
            for (int j = 0; j < kSemOB; ++j)
                if (o0 + j < k.ohi) a.prod[((int64_t)k.slot * a.sw + o0 + j) * a.N2 + i] = acc[j];
    }
    __threadfence_block();
    __syncthreads();
    if (wave != 0 || !valid || scores == nullptr) return;
    const int64_t N2 = a.N2;
    const float* P = a.prod + i;
    float e = 0.f;
    if constexpr (MODEL == KGE_SLM) {
        const float* rn = X + sem_region_off(1, a.de, a.dr) + lane;
        for (int j = 0; j < a.dr; ++j) {
            const float u = P[(int64_t)j * N2] + P[(int64_t)(a.sw + j) * N2];
            e = fmaf(rn[j * kSemLd], tanhf(u), e);
        }
        scores[i] = -e;
    } else {
        const int d = a.de;
        for (int c = 0; c < d; ++c) {
            const float A = P[(int64_t)c * N2], B = P[(int64_t)(d + c) * N2];
            const float C = P[(int64_t)(2 * d + c) * N2], D = P[(int64_t)(3 * d + c) * N2];
            const float gu = MODEL == KGE_SME ? (A + B) + a.bu[c] : A * B + a.bu[c];
            const float gv = MODEL == KGE_SME ? (C + D) + a.bv[c] : C * D + a.bv[c];
            e = fmaf(gu, gv, e);
        }
        scores[i] = MODEL == KGE_SME ? -e : e;
    }
}

// transposed products of the backward: dx^_c = sum over terms of sum_o W(o, c) dX_slot[o], c in [clo, chi)
struct SemBTask { int target, clo, chi, nterm, dout, so, sc; int slot[2]; const float* W[2]; };

template <int MODEL>
__device__ __forceinline__ SemBTask sem_bwd_task(const SemArgs& a, int wave) {
    SemBTask k;
    if constexpr (MODEL == KGE_SLM) {   // dh^ = M1 du, dt^ = M2 du (du in slot 0): (o = j, c) = M[c][j]
        const int half = (a.de + 1) / 2;
        k.target = wave < 2 ? 0 : 2; k.nterm = 1; k.slot[0] = 0; k.W[0] = wave < 2 ? a.W[0] : a.W[1];
        k.slot[1] = 0; k.W[1] = k.W[0];
        k.clo = (wave & 1) ? half : 0; k.chi = (wave & 1) ? a.de : half;
        k.dout = a.dr; k.so = 1; k.sc = a.dr;
    } else {                            // dh^ = mu1^T dA, dt^ = mv1^T dC, dr^ = mu2^T dB + mv2^T dD (split over waves 1 / 3)
        const int d = a.de, half = (d + 1) / 2;
        k.dout = d; k.so = d; k.sc = 1;
        if (wave == 0 || wave == 2) {
            k.target = wave; k.nterm = 1; k.slot[0] = wave; k.W[0] = a.W[wave]; k.slot[1] = wave; k.W[1] = a.W[wave];
            k.clo = 0; k.chi = d;
        } else {
            k.target = 1; k.nterm = 2; k.slot[0] = 1; k.W[0] = a.W[1]; k.slot[1] = 3; k.W[1] = a.W[3];
            k.clo = wave == 1 ? 0 : half; k.chi = wave == 1 ? half : d;
        }
    }
    return k;
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_sem_backward(SemArgs a, const float* __restrict__ dscore, float* __restrict__ gent,
                                                      float* __restrict__ grel) {
    extern __shared__ float X[];
    const int T = sem_tiles_floats(a.de, a.dr);
    float* DY = X + T;                     // dL/dx^ tiles, same regions
    float* sdot = DY + T;                  // [3][64]: x^ . dL/dx^ per input and triple
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile0 = (int64_t)blockIdx.x * kSemTile;
    const int64_t i = tile0 + lane;
    const bool valid = i < a.N2;
    const int64_t N2 = a.N2;
    sem_load_inputs(a, X, i, valid, wave, lane, false);
    const float g = valid ? dscore[i] : 0.f;
    // 1. hidden-layer gradients, elementwise (all four waves, k interleaved), over the products in place
    float* P = a.prod + i;
    if constexpr (MODEL == KGE_SLM) {
        __syncthreads();   // r^ tile
        const float* rn = X + sem_region_off(1, a.de, a.dr) + lane;
        float* dr_ = DY + sem_region_off(1, a.de, a.dr) + lane;
        for (int j = wave; j < a.dr; j += 4) {
            float du = 0.f, drv = 0.f;
            if (valid) {
                const float th = tanhf(P[(int64_t)j * N2] + P[(int64_t)(a.sw + j) * N2]);
                const float gn = -g;
                drv = gn * th;
                du = gn * rn[j * kSemLd] * (1.0f - th * th);
                P[(int64_t)j * N2] = du;
            }
            dr_[j * kSemLd] = drv;
        }
    } else {
        const int d = a.de;
        if (valid) {
            for (int c = wave; c < d; c += 4) {
                const float A = P[(int64_t)c * N2], B = P[(int64_t)(d + c) * N2];
                const float C = P[(int64_t)(2 * d + c) * N2], D = P[(int64_t)(3 * d + c) * N2];
                float dA, dB, dC, dD, dgu, dgv;
                if constexpr (MODEL == KGE_SME) {
                    const float gu = (A + B) + a.bu[c], gv = (C + D) + a.bv[c];
                    dgu = -g * gv; dgv = -g * gu;
                    dA = dgu; dB = dgu; dC = dgv; dD = dgv;
                } else {
                    const float gu = A * B + a.bu[c], gv = C * D + a.bv[c];
                    dgu = g * gv; dgv = g * gu;
                    dA = dgu * B; dB = dgu * A; dC = dgv * D; dD = dgv * C;
                }
                P[(int64_t)c * N2] = dA; P[(int64_t)(d + c) * N2] = dB;
                P[(int64_t)(2 * d + c) * N2] = dC; P[(int64_t)(3 * d + c) * N2] = dD;
                P[(int64_t)(4 * d + c) * N2] = dgu; P[(int64_t)(5 * d + c) * N2] = dgv;
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    // 2. transposed products into the DY tiles
    const SemBTask k = sem_bwd_task<MODEL>(a, wave);
    float* dy = DY + sem_region_off(k.target, a.de, a.dr) + lane;
    for (int c0 = k.clo; c0 < k.chi; c0 += kSemOB) {
        float acc[kSemOB];
#pragma unroll
        for (int j = 0; j < kSemOB; ++j) acc[j] = 0.f;
        for (int tm = 0; tm < k.nterm; ++tm) {
            const float* src = a.prod + (int64_t)k.slot[tm] * a.sw * N2 + (valid ? i : 0);
            const float* W = k.W[tm];
            for (int o = 0; o < k.dout; ++o) {
                const float dx = valid ? src[(int64_t)o * N2] : 0.f;
#pragma unroll
                for (int j = 0; j < kSemOB; ++j) {
                    const int c = min(c0 + j, k.chi - 1);
                    acc[j] = fmaf(W[(int64_t)o * k.so + (int64_t)c * k.sc], dx, acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kSemOB; ++j)
            if (c0 + j < k.chi) dy[(c0 + j) * kSemLd] = acc[j];
    }
    __syncthreads();
    // 3. normalisation backward (dx = inv (dx^ - x^ (x^ . dx^)); the clamped branch of F.normalize: dx = inv dx^) and the
    //    scatter: wave s owns input s; lanes walk a row's elements so that each atomic burst is one contiguous row
    if (wave >= 3) return;
    const int w = wave == 1 ? a.dr : a.de;
    const float* xs = X + sem_region_off(wave, a.de, a.dr);
    const float* ds = DY + sem_region_off(wave, a.de, a.dr);
    float dot = 0.f;
    for (int c = 0; c < w; ++c) dot = fmaf(xs[c * kSemLd + lane], ds[c * kSemLd + lane], dot);
    const float inv_l = valid ? a.inv[wave * N2 + i] : 0.f;
    sdot[wave * 64 + lane] = inv_l >= 1.0f / kEpsNormalize ? 0.f : dot;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // sdot[s][*] is written and read by wave s alone
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float* G = wave == 1 ? grel : gent;
    const int ntr = (int)min((int64_t)kSemTile, N2 - tile0);
    for (int ii = 0; ii < ntr; ++ii) {
        const int64_t ti = tile0 + ii;
        const int64_t id = wave == 0 ? a.h.at(ti) : wave == 1 ? a.r.at(ti) : a.t.at(ti);
        const float inv = a.inv[wave * N2 + ti], dt = sdot[wave * 64 + ii];
        for (int c = lane; c < w; c += 64)
            atomicAdd(G + id * w + c, inv * (ds[c * kSemLd + ii] - xs[c * kSemLd + ii] * dt));
    }
}

// ---------------------------------------------------------------- shared-matrix gradients: per-chunk partials + ordered sum
// source of one side of an outer product: 0 / 1 / 2 = the normalised h / r / t row, 3 = product slot `slot`, 4 = the constant 1
struct WSide { int kind, slot, len; };
struct WTask { WSide L, R; int64_t off; };   // gradient[a][b] = sum_i L_i[a] R_i[b], rows = L.len, cols = R.len, at part + off
struct WArgs {
    SemArgs a;
    WTask task[6];
    int64_t wsize, csz;
    int pairs;   // [positives | negatives]: walk the batch as pos 0, neg 0, pos 1, ... so that the two halves of a pair meet early
    float* part;
};

__device__ __forceinline__ float wside_val(const SemArgs& a, const WSide& s, int k, int64_t i) {
    if (s.kind == 4) return 1.0f;
    if (s.kind == 3) return a.prod[((int64_t)s.slot * a.sw + k) * a.N2 + i];
    const int64_t id = s.kind == 0 ? a.h.at(i) : s.kind == 1 ? a.r.at(i) : a.t.at(i);
    const float* tab = s.kind == 1 ? a.rel : a.ent;
    return tab[id * s.len + k] * a.inv[s.kind * a.N2 + i];
}

__global__ __launch_bounds__(256) void k_sem_wgrad(WArgs w) {
    constexpr int LP = kSemMaxDim + 4;
    __shared__ float Ls[kSub][LP], Rs[kSub][LP];
    const WTask tk = w.task[blockIdx.z];
    const int rows = tk.L.len, cols = tk.R.len;
    const int BR = (rows + 3) / 4, BC = (cols + 3) / 4;
    const int b = blockIdx.y * 256 + threadIdx.x;
    const bool own = b < BR * BC;
    const int br = own ? b / BC : 0, bc = own ? b % BC : 0;
    const int64_t lo = (int64_t)blockIdx.x * w.csz, hi = min(w.a.N2, lo + w.csz);
    // a gradient entry is a sum of up to 2n terms of both signs that largely cancel (a positive's and its negative's share of
    // the bias: SME_BL's bu / bv at B = 50 000 sum to ~10 from terms whose one-sided partial sums reach ~1e4): the pairs are
    // walked interleaved, and each 32-triple stage is summed on its own before it joins the running total
    float acc[4][4], tot[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) tot[x][y] = 0.f;
    for (int64_t s0 = lo; s0 < hi; s0 += kSub) {
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[x][y] = 0.f;
        for (int idx = threadIdx.x; idx < kSub * LP; idx += 256) {
            // slots are SoA over the triples (triple fastest), table rows are contiguous (element fastest)
            const bool tri_fast = tk.L.kind == 3;
            const int ii = tri_fast ? idx % kSub : idx / LP, k = tri_fast ? idx / kSub : idx % LP;
            const int64_t pi = s0 + ii, ti = w.pairs ? ((pi & 1) ? (w.a.N2 >> 1) + (pi >> 1) : (pi >> 1)) : pi;
            Ls[ii][k] = (k < rows && pi < hi) ? wside_val(w.a, tk.L, k, ti) : 0.f;
        }
        for (int idx = threadIdx.x; idx < kSub * LP; idx += 256) {
            const bool tri_fast = tk.R.kind == 3;
            const int ii = tri_fast ? idx % kSub : idx / LP, k = tri_fast ? idx / kSub : idx % LP;
            const int64_t pi = s0 + ii, ti = w.pairs ? ((pi & 1) ? (w.a.N2 >> 1) + (pi >> 1) : (pi >> 1)) : pi;
            Rs[ii][k] = (k < cols && pi < hi) ? wside_val(w.a, tk.R, k, ti) : 0.f;
        }
        __syncthreads();
        if (own) {
            for (int ii = 0; ii < kSub; ++ii) {
                float l[4], r[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) { l[x] = Ls[ii][br * 4 + x]; r[x] = Rs[ii][bc * 4 + x]; }
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) acc[x][y] = fmaf(l[x], r[y], acc[x][y]);
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) tot[x][y] += acc[x][y];
        }
        __syncthreads();
    }
    if (!own) return;
    float* out = w.part + (int64_t)blockIdx.x * w.wsize + tk.off;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int ra = br * 4 + x, cb = bc * 4 + y;
            if (ra < rows && cb < cols) out[(int64_t)ra * cols + cb] = tot[x][y];
        }
}

struct WDest { float* g[6]; int64_t off[7]; int ntask; };

__global__ __launch_bounds__(256) void k_sem_wreduce(const float* __restrict__ part, int64_t wsize, int nchunk, WDest d) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= wsize) return;
    float s = 0.f;   // chunk order, in groups of 8 (shorter chains, same fixed order every run)
    for (int p0 = 0; p0 < nchunk; p0 += 8) {
        float g = 0.f;
        for (int p = p0; p < min(nchunk, p0 + 8); ++p) g += part[(int64_t)p * wsize + e];
        s += g;
    }
    int t = 0;
    while (t + 1 < d.ntask && e >= d.off[t + 1]) ++t;
    d.g[t][e - d.off[t]] += s;
}

// ---------------------------------------------------------------- host side: train
static SemArgs sem_args(const kge_model_desc* m, const SemShape& s, IdSplit h, IdSplit r, IdSplit t, int64_t N2, const SemWs& w) {
    SemArgs a;
    a.ent = m->tables[0]; a.rel = m->tables[1];
    if (is_sme(m->model)) {
        a.W[0] = m->tables[2]; a.W[1] = m->tables[3]; a.W[2] = m->tables[5]; a.W[3] = m->tables[6];
        a.bu = m->tables[4]; a.bv = m->tables[7];
    } else {
        a.W[0] = m->tables[2]; a.W[1] = m->tables[3]; a.W[2] = nullptr; a.W[3] = nullptr;
        a.bu = nullptr; a.bv = nullptr;
    }
    a.h = h; a.r = r; a.t = t; a.N2 = N2;
    a.de = s.de; a.dr = s.dr; a.sw = s.sw;
    a.inv = w.inv; a.prod = w.prod;
    return a;
}

static size_t sem_lds(const SemShape& s, bool backward) {
    const size_t T = (size_t)(2 * s.de + s.dr) * kSemLd;
    return (backward ? 2 * T + 3 * 64 : T) * sizeof(float);
}

// the LDS limit of the six train kernels is raised once, to the largest size (kSemMaxDim): no call inside a graph capture
static void sem_lds_attr() {
    static const bool done = [] {
        const int most = (int)((size_t)(2 * 3 * kSemMaxDim * kSemLd + 3 * 64) * sizeof(float));
        const void* k[6] = {(const void*)k_sem_forward<KGE_SLM>, (const void*)k_sem_forward<KGE_SME>,
                            (const void*)k_sem_forward<KGE_SME_BL>, (const void*)k_sem_backward<KGE_SLM>,
                            (const void*)k_sem_backward<KGE_SME>, (const void*)k_sem_backward<KGE_SME_BL>};
        bool ok = true;
        for (const void* f : k) ok = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, most) == hipSuccess && ok;
        return ok;
    }();
    (void)done;
}

static int sem_forward_run(const kge_model_desc* m, IdSplit h, IdSplit r, IdSplit t, int64_t N2, float* scores, void* ws,
                           size_t ws_bytes, hipStream_t st) {
    if (sem_check(m, "kge (SLM / SME)")) return -1;
    const SemShape s = sem_shape(m);
    const SemWs w = sem_carve(s, N2, ws);
    if (!ws || ws_bytes < w.bytes) { set_error("kge (SLM / SME): workspace too small (%zu < %zu)", ws_bytes, w.bytes); return -1; }
    const SemArgs a = sem_args(m, s, h, r, t, N2, w);
    const size_t lds = sem_lds(s, false);
    sem_lds_attr();
    const dim3 grid((unsigned)((N2 + kSemTile - 1) / kSemTile));
    switch (m->model) {
        case KGE_SLM: hipLaunchKernelGGL(k_sem_forward<KGE_SLM>, grid, dim3(256), lds, st, a, scores); break;
        case KGE_SME: hipLaunchKernelGGL(k_sem_forward<KGE_SME>, grid, dim3(256), lds, st, a, scores); break;
        default: hipLaunchKernelGGL(k_sem_forward<KGE_SME_BL>, grid, dim3(256), lds, st, a, scores); break;
    }
    return check_launch("k_sem_forward");
}

// after sem_forward_run on the same ids and workspace: row gradients (atomics) + shared-matrix gradients (ordered partials)
static int sem_backward_run(const kge_model_desc* m, IdSplit h, IdSplit r, IdSplit t, int64_t N2, const float* dscore, void* ws,
                            bool pairs, hipStream_t st) {
    const SemShape s = sem_shape(m);
    const SemWs w = sem_carve(s, N2, ws);
    const SemArgs a = sem_args(m, s, h, r, t, N2, w);
    const size_t lds = sem_lds(s, true);
    sem_lds_attr();
    const dim3 grid((unsigned)((N2 + kSemTile - 1) / kSemTile));
    float* ge = m->grads[0];
    float* gr = m->grads[1];
    switch (m->model) {
        case KGE_SLM: hipLaunchKernelGGL(k_sem_backward<KGE_SLM>, grid, dim3(256), lds, st, a, dscore, ge, gr); break;
        case KGE_SME: hipLaunchKernelGGL(k_sem_backward<KGE_SME>, grid, dim3(256), lds, st, a, dscore, ge, gr); break;
        default: hipLaunchKernelGGL(k_sem_backward<KGE_SME_BL>, grid, dim3(256), lds, st, a, dscore, ge, gr); break;
    }
    WArgs wa;
    wa.a = a; wa.wsize = s.wsize; wa.part = w.part; wa.pairs = pairs ? 1 : 0;
    WDest dd;
    dd.ntask = s.ntask;
    const int d = s.de;
    if (is_sme(m->model)) {
        const int in_of[4] = {0, 1, 2, 1};
        const int tab_of[6] = {2, 3, 5, 6, 4, 7};
        int64_t off = 0;
        for (int k = 0; k < 6; ++k) {
            WTask& tk = wa.task[k];
            tk.L = WSide{3, k, d};
            tk.R = k < 4 ? WSide{in_of[k], 0, d} : WSide{4, 0, 1};
            tk.off = off; dd.off[k] = off; dd.g[k] = m->grads[tab_of[k]];
            off += (int64_t)tk.L.len * tk.R.len;
        }
        dd.off[6] = off;
    } else {
        for (int k = 0; k < 2; ++k) {
            WTask& tk = wa.task[k];
            tk.L = WSide{k == 0 ? 0 : 2, 0, s.de};
            tk.R = WSide{3, 0, s.dr};
            tk.off = (int64_t)k * s.de * s.dr; dd.off[k] = tk.off; dd.g[k] = m->grads[2 + k];
        }
        dd.off[2] = s.wsize;
        for (int k = 2; k < 6; ++k) { wa.task[k] = wa.task[0]; dd.g[k] = nullptr; dd.off[k + 1] = s.wsize; }
    }
    int64_t csz = (N2 + kChunks - 1) / kChunks;
    if (csz < kSub) csz = kSub;
    wa.csz = csz;
    const int nchunk = (int)((N2 + csz - 1) / csz);
    int maxblocks = 0;
    for (int k = 0; k < s.ntask; ++k) {
        const int nb = ((wa.task[k].L.len + 3) / 4) * ((wa.task[k].R.len + 3) / 4);
        if (nb > maxblocks) maxblocks = nb;
    }
    hipLaunchKernelGGL(k_sem_wgrad, dim3((unsigned)nchunk, (unsigned)((maxblocks + 255) / 256), (unsigned)s.ntask), dim3(256), 0, st, wa);
    hipLaunchKernelGGL(k_sem_wreduce, dim3((unsigned)((s.wsize + 255) / 256)), dim3(256), 0, st, (const float*)w.part, s.wsize, nchunk, dd);
    return check_launch("k_sem_backward / k_sem_wgrad");
}

int launch_semantic_forward(const kge_model_desc* m, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n,
                            float* scores, void* ws, size_t ws_bytes, hipStream_t s) {
    return sem_forward_run(m, id_whole(h, n), id_whole(r, n), id_whole(t, n), n, scores, ws, ws_bytes, s);
}

int launch_semantic_backward(const kge_model_desc* m, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n,
                             const float* dscore, void* ws, size_t ws_bytes, hipStream_t s) {
    if (int rc = sem_forward_run(m, id_whole(h, n), id_whole(r, n), id_whole(t, n), n, nullptr, ws, ws_bytes, s)) return rc;
    return sem_backward_run(m, id_whole(h, n), id_whole(r, n), id_whole(t, n), n, dscore, ws, false, s);
}

int launch_semantic_pair_forward(const kge_model_desc* m, const int64_t* ph, const int64_t* pr, const int64_t* pt,
                                 const int64_t* nh, const int64_t* nr, const int64_t* nt, int64_t n, float* scores2, void* ws,
                                 size_t ws_bytes, hipStream_t s) {
    return sem_forward_run(m, IdSplit{ph, nh, n}, IdSplit{pr, nr, n}, IdSplit{pt, nt, n}, 2 * n, scores2, ws, ws_bytes, s);
}

int launch_semantic_pair_backward(const kge_model_desc* m, const int64_t* ph, const int64_t* pr, const int64_t* pt,
                                  const int64_t* nh, const int64_t* nr, const int64_t* nt, int64_t n, const float* dscore2,
                                  void* ws, size_t ws_bytes, hipStream_t s) {
    (void)ws_bytes;   // checked by the forward on the same layout
    return sem_backward_run(m, IdSplit{ph, nh, n}, IdSplit{pr, nr, n}, IdSplit{pt, nt, n}, 2 * n, dscore2, ws, true, s);
}

// ---------------------------------------------------------------- SME / SME_BL rank: query contraction + the negated-dot sweep
// candidate rows [e^ | 1], K = d + 1
__global__ __launch_bounds__(256) void k_sem_cand(const float* __restrict__ ent, int64_t E, int d, float* __restrict__ cand) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    const float* x = ent + e * d;
    float n2 = 0.f;
    for (int c = lane; c < d; c += 64) n2 = fmaf(x[c], x[c], n2);
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(n2)), kEpsNormalize);
    float* o = cand + e * (d + 1);
    for (int c = lane; c < d; c += 64) o[c] = x[c] * inv;
    if (lane == 0) o[d] = 1.0f;
}

// one workgroup per test triple: query rows [2i] = tail sweep, [2i + 1] = head sweep, each [q | c] of width d + 1 with
// energy(e) = -([q | c] . [e^ | 1])  (the pipeline's negated dot)
template <int MODEL>
__global__ __launch_bounds__(256) void k_sem_queries(const kge_model_desc md, const int64_t* __restrict__ triples, int64_t n,
                                                     float* __restrict__ qrows) {
    __shared__ float xh[kSemMaxDim], xr[kSemMaxDim], xt[kSemMaxDim];
    __shared__ float m1h[kSemMaxDim], m2r[kSemMaxDim], m1t[kSemMaxDim], m2rv[kSemMaxDim];   // mu1 h^, mu2 r^, mv1 t^, mv2 r^
    __shared__ float wu[kSemMaxDim], wv[kSemMaxDim], red[2][8];
    const int d = md.dim, tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    const float *ent = md.tables[0], *rel = md.tables[1], *mu1 = md.tables[2], *mu2 = md.tables[3], *bu = md.tables[4];
    const float *mv1 = md.tables[5], *mv2 = md.tables[6], *bv = md.tables[7];
    const int64_t h = triples[3 * i], r = triples[3 * i + 1], t = triples[3 * i + 2];
    if (tid < 192) {   // waves 0 / 1 / 2: normalise h / r / t
        const int wv_ = tid >> 6, lane = tid & 63;
        const float* x = (wv_ == 1 ? rel + r * d : ent + (wv_ == 0 ? h : t) * d);
        float n2 = 0.f;
        for (int c = lane; c < d; c += 64) n2 = fmaf(x[c], x[c], n2);
        const float inv = 1.0f / fmaxf(sqrtf(wave_sum(n2)), kEpsNormalize);
        float* o = wv_ == 0 ? xh : wv_ == 1 ? xr : xt;
        for (int c = lane; c < d; c += 64) o[c] = x[c] * inv;
    }
    __syncthreads();
    for (int k = tid; k < 4 * d; k += 256) {   // the four matrix-vector products M @ x
        const int which = k / d, o = k % d;
        const float* M = which == 0 ? mu1 : which == 1 ? mu2 : which == 2 ? mv1 : mv2;
        const float* x = which == 0 ? xh : which == 2 ? xt : xr;
        float acc = 0.f;
        for (int c = 0; c < d; ++c) acc = fmaf(M[(int64_t)o * d + c], x[c], acc);
        (which == 0 ? m1h : which == 1 ? m2r : which == 2 ? m1t : m2rv)[o] = acc;
    }
    __syncthreads();
    // tail side: wu = the vector mv1^T is applied to, cu = the query constant; head side: wv, cv.
    //   SME:    gu = m1h + m2r + bu;  tail q = -(mv1^T gu), c = -(gu . (m2rv + bv))  -> energy = -(q'.t^ + c') with q' = mv1^T gu
    //   SME_BL: gu = m1h * m2r + bu;  tail energy = (mv1^T (gu * m2rv)) . t^ + gu . bv
    float pu = 0.f, pv = 0.f;
    for (int k = tid; k < d; k += 256) {
        float gu, gv;
        if constexpr (MODEL == KGE_SME) {
            gu = (m1h[k] + m2r[k]) + bu[k]; gv = (m1t[k] + m2rv[k]) + bv[k];
            wu[k] = gu; wv[k] = gv;
            pu = fmaf(gu, m2rv[k] + bv[k], pu);   // tail constant: gu . (mv2 r^ + bv)
            pv = fmaf(gv, m2r[k] + bu[k], pv);    // head constant: gv . (mu2 r^ + bu)
        } else {
            gu = m1h[k] * m2r[k] + bu[k]; gv = m1t[k] * m2rv[k] + bv[k];
            wu[k] = gu * m2rv[k]; wv[k] = gv * m2r[k];
            pu = fmaf(gu, bv[k], pu);
            pv = fmaf(gv, bu[k], pv);
        }
    }
    pu = wave_sum(pu); pv = wave_sum(pv);
    if ((tid & 63) == 0) { red[0][tid >> 6] = pu; red[1][tid >> 6] = pv; }
    __syncthreads();
    // NEGDOT energy = -(row . cand): SME rows are +[q | c] (energy = -(q . e^ + c)), SME_BL rows are -[q | c]
    constexpr float sg = MODEL == KGE_SME ? 1.0f : -1.0f;
    float* qt = qrows + (2 * i) * (int64_t)(d + 1);
    float* qh = qt + (d + 1);
    for (int c = tid; c < 2 * d; c += 256) {
        const int side = c / d, cc = c % d;
        const float* M = side == 0 ? mv1 : mu1;
        const float* wvec = side == 0 ? wu : wv;
        float acc = 0.f;
        for (int k = 0; k < d; ++k) acc = fmaf(M[(int64_t)k * d + cc], wvec[k], acc);   // (M^T w)[cc]
        (side == 0 ? qt : qh)[cc] = sg * acc;
    }
    if (tid == 0) {
        qt[d] = sg * (red[0][0] + red[0][1] + red[0][2] + red[0][3]);
        qh[d] = sg * (red[1][0] + red[1][1] + red[1][2] + red[1][3]);
    }
}

// ---------------------------------------------------------------- SLM rank
struct SlmEvalWs { float *P1, *P2, *qlin, *qr, *scores; int64_t* truth; int32_t *rank, *frank; int chunk; int64_t Ep; size_t bytes; };

static void slm_eval_plan(const kge_model_desc* m, int64_t n, void* ws, SlmEvalWs* w) {
    size_t off = 0;
    char* base = (char*)ws;
    auto take = [&](size_t b) { char* p = base ? base + off : nullptr; off += align256(b); return p; };
    const int64_t E = m->tot_entity;
    const int kr = m->rel_dim;
    w->chunk = (int)(n < kSlmChunk ? (n < 1 ? 1 : n) : kSlmChunk);
    w->Ep = E;
    const int64_t C = w->chunk;
    w->P1 = (float*)take((size_t)kr * E * 4);   // d_r-major: P1[j * E + e]
    w->P2 = (float*)take((size_t)kr * E * 4);
    w->qlin = (float*)take((size_t)2 * C * kr * 4);
    w->qr = (float*)take((size_t)2 * C * kr * 4);
    w->scores = (float*)take((size_t)2 * C * E * 4);
    w->truth = (int64_t*)take((size_t)2 * C * 8);
    w->rank = nullptr; w->frank = nullptr;
    w->bytes = off;
}

// P1 = E^ M1, P2 = E^ M2, one wave per entity row
__global__ __launch_bounds__(256) void k_slm_ent_tables(const float* __restrict__ ent, const float* __restrict__ M1,
                                                        const float* __restrict__ M2, int64_t E, int d, int kr,
                                                        float* __restrict__ P1, float* __restrict__ P2) {
    __shared__ float sx[4][kSemMaxDim];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 4 + wave;
    if (e >= E) return;
    const float* x = ent + e * d;
    float n2 = 0.f;
    for (int c = lane; c < d; c += 64) n2 = fmaf(x[c], x[c], n2);
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(n2)), kEpsNormalize);
    for (int c = lane; c < d; c += 64) sx[wave][c] = x[c] * inv;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int j = lane; j < kr; j += 64) {
        float a1 = 0.f, a2 = 0.f;
        for (int c = 0; c < d; ++c) {
            a1 = fmaf(sx[wave][c], M1[(int64_t)c * kr + j], a1);
            a2 = fmaf(sx[wave][c], M2[(int64_t)c * kr + j], a2);
        }
        P1[(int64_t)j * E + e] = a1;
        P2[(int64_t)j * E + e] = a2;
    }
}

// per chunk triple i: rows 2i (tail sweep: a = h^ M1) and 2i + 1 (head sweep: b = t^ M2), r^, truth
__global__ __launch_bounds__(256) void k_slm_q_prep(const float* __restrict__ ent, const float* __restrict__ rel,
                                                    const float* __restrict__ M1, const float* __restrict__ M2,
                                                    const int64_t* __restrict__ triples, int64_t n, int d, int kr, SlmEvalWs w) {
    __shared__ float sh[4][kSemMaxDim], st[4][kSemMaxDim];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= n) return;
    const int64_t h = triples[3 * i], r = triples[3 * i + 1], t = triples[3 * i + 2];
    const float* eh = ent + h * d; const float* et = ent + t * d; const float* er = rel + r * kr;
    float nh = 0.f, nt = 0.f, nr = 0.f;
    for (int c = lane; c < d; c += 64) { nh = fmaf(eh[c], eh[c], nh); nt = fmaf(et[c], et[c], nt); }
    for (int c = lane; c < kr; c += 64) nr = fmaf(er[c], er[c], nr);
    const float ih = 1.0f / fmaxf(sqrtf(wave_sum(nh)), kEpsNormalize), it = 1.0f / fmaxf(sqrtf(wave_sum(nt)), kEpsNormalize);
    const float ir = 1.0f / fmaxf(sqrtf(wave_sum(nr)), kEpsNormalize);
    for (int c = lane; c < d; c += 64) { sh[wave][c] = eh[c] * ih; st[wave][c] = et[c] * it; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int j = lane; j < kr; j += 64) {
        float a = 0.f, b = 0.f;
        for (int c = 0; c < d; ++c) {
            a = fmaf(sh[wave][c], M1[(int64_t)c * kr + j], a);
            b = fmaf(st[wave][c], M2[(int64_t)c * kr + j], b);
        }
        w.qlin[(2 * i) * kr + j] = a; w.qlin[(2 * i + 1) * kr + j] = b;
        const float rn = er[j] * ir;
        w.qr[(2 * i) * kr + j] = rn; w.qr[(2 * i + 1) * kr + j] = rn;
    }
    if (lane == 0) { w.truth[2 * i] = t; w.truth[2 * i + 1] = h; }
}

// energies of query row q (blockIdx.y) against 256 candidates per workgroup: thread = candidate, the query in LDS
__global__ __launch_bounds__(256) void k_slm_sweep(int64_t E, int kr, SlmEvalWs w, float* __restrict__ scores) {
    __shared__ float sl[kSemMaxDim], sr[kSemMaxDim];
    const int64_t q = blockIdx.y;
    for (int j = threadIdx.x; j < kr; j += 256) { sl[j] = w.qlin[q * kr + j]; sr[j] = w.qr[q * kr + j]; }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float* P = (q & 1) == 0 ? w.P2 : w.P1;   // tail sweep: candidates' t^ M2; head sweep: candidates' h^ M1
    float acc = 0.f;
    if ((q & 1) == 0)
        for (int j = 0; j < kr; ++j) acc = fmaf(sr[j], tanhf(sl[j] + P[(int64_t)j * E + e]), acc);
    else
        for (int j = 0; j < kr; ++j) acc = fmaf(sr[j], tanhf(P[(int64_t)j * E + e] + sl[j]), acc);
    scores[q * E + e] = -acc;
}

__global__ void k_slm_rank_rows(const float* __restrict__ scores, int64_t c, int64_t E, const int64_t* __restrict__ truth,
                                const int64_t* __restrict__ tail_off, const int32_t* __restrict__ tail_ids,
                                const int64_t* __restrict__ head_off, const int32_t* __restrict__ head_ids, int64_t tri0,
                                int64_t n_total, int32_t* __restrict__ ranks) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= 2 * c) return;
    const int64_t i = q >> 1;
    const int side = (int)(q & 1);
    const float* s = scores + q * E;
    const int64_t tr = truth[q];
    const float stv = s[tr];
    int cnt = 0, fc = 0;
    for (int64_t e = lane; e < E; e += 64) cnt += s[e] < stv ? 1 : 0;
    const int64_t* off = side == 0 ? tail_off : head_off;
    const int32_t* ids = side == 0 ? tail_ids : head_ids;
    if (off)
        for (int64_t j = off[tri0 + i] + lane; j < off[tri0 + i + 1]; j += 64) {
            const int64_t e = ids[j];
            fc += (e != tr && s[e] < stv) ? 1 : 0;
        }
    cnt = (int)wave_sum((float)cnt);
    fc = (int)wave_sum((float)fc);
    if (lane == 0) {
        ranks[(side == 0 ? 1 : 0) * n_total + tri0 + i] = cnt;   // rows: head, tail, fhead, ftail
        ranks[(side == 0 ? 3 : 2) * n_total + tri0 + i] = cnt - fc;
    }
}

static int slm_eval(const kge_model_desc* m, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                    const int64_t* head_off, const int32_t* head_ids, void* ws, size_t ws_bytes, int32_t* ranks, int32_t* ties,
                    float* scores_out, hipStream_t s) {
    SlmEvalWs w;
    slm_eval_plan(m, n, ws, &w);
    if (!ws || ws_bytes < w.bytes) { set_error("kge_eval (SLM): workspace too small (%zu < %zu)", ws_bytes, w.bytes); return -1; }
    if (n <= 0) return 0;
    const int64_t E = m->tot_entity;
    const int d = m->dim, kr = m->rel_dim;
    if (ties) (void)hipMemsetAsync(ties, 0xFF, (size_t)2 * n * sizeof(int32_t), s);   // (ties are not counted: -1)
    hipLaunchKernelGGL(k_slm_ent_tables, dim3((unsigned)((E + 3) / 4)), dim3(256), 0, s, m->tables[0], m->tables[2], m->tables[3],
                       E, d, kr, w.P1, w.P2);
    for (int64_t lo = 0; lo < n; lo += w.chunk) {
        const int64_t c = min((int64_t)w.chunk, n - lo);
        hipLaunchKernelGGL(k_slm_q_prep, dim3((unsigned)((c + 3) / 4)), dim3(256), 0, s, m->tables[0], m->tables[1], m->tables[2],
                           m->tables[3], triples + 3 * lo, c, d, kr, w);
        float* sc = scores_out ? scores_out + 2 * lo * E : w.scores;
        hipLaunchKernelGGL(k_slm_sweep, dim3((unsigned)((E + 255) / 256), (unsigned)(2 * c)), dim3(256), 0, s, E, kr, w, sc);
        if (ranks)
            hipLaunchKernelGGL(k_slm_rank_rows, dim3((unsigned)((2 * c + 3) / 4)), dim3(256), 0, s, sc, c, E, w.truth, tail_off,
                               tail_ids, head_off, head_ids, lo, n, ranks);
    }
    return check_launch("SLM sweep");
}

// ---------------------------------------------------------------- host side: rank entry points (called from kge_eval.hip)
size_t semantic_eval_workspace_bytes(const kge_model_desc* m, int64_t n) {
    if (m->model == KGE_SLM) { SlmEvalWs w; slm_eval_plan(m, n, nullptr, &w); return w.bytes; }
    return dot_rows_plan(nullptr, m->tot_entity, n, m->dim + 1).bytes;
}

int launch_semantic_eval(const kge_model_desc* m, const int64_t* triples, int64_t n, const int64_t* tail_off,
                         const int32_t* tail_ids, const int64_t* head_off, const int32_t* head_ids, void* ws, size_t ws_bytes,
                         int32_t* ranks, int32_t* ties, float* scores, hipStream_t s, int side) {
    if (sem_check(m, "kge_eval")) return -1;
    if (m->model == KGE_SLM) {
        if (side != 2) { set_error("kge_eval_sweep_scores_side: the SLM sweep computes both sides per call"); return -1; }
        return slm_eval(m, triples, n, tail_off, tail_ids, head_off, head_ids, ws, ws_bytes, ranks, ties, scores, s);
    }
    const DotRowsPlan w = dot_rows_plan(ws, m->tot_entity, n, m->dim + 1);
    if (!ws || ws_bytes < w.bytes) { set_error("kge_eval (SME): workspace too small (%zu < %zu)", ws_bytes, w.bytes); return -1; }
    if (n <= 0) return 0;
    const int64_t E = m->tot_entity;
    hipLaunchKernelGGL(k_sem_cand, dim3((unsigned)((E + 3) / 4)), dim3(256), 0, s, m->tables[0], E, m->dim, w.cand);
    if (m->model == KGE_SME)
        hipLaunchKernelGGL(k_sem_queries<KGE_SME>, dim3((unsigned)n), dim3(256), 0, s, *m, triples, n, w.qrows);
    else
        hipLaunchKernelGGL(k_sem_queries<KGE_SME_BL>, dim3((unsigned)n), dim3(256), 0, s, *m, triples, n, w.qrows);
    if (int rc = check_launch("k_sem_queries")) return rc;
    return launch_dot_eval(w.cand, w.qrows, m->dim + 1, E, triples, n, tail_off, tail_ids, head_off, head_ids, w.pipe, w.pipe_bytes,
                           ranks, ties, scores, s, side);
}

}  // namespace kge
