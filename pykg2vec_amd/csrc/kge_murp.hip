// kge_murp.hip -- MuRP (pointwise.py:1004-1133) as the reference executes it, in float64 throughout.
//
//   h', t', r' = clip(ent[h]), clip(ent[t]), clip(rel[r])        clip(x) = x / (|x| - 1e-5) where |x| >= 1
//   u_e = arsech(c) h' / c,  c = clamp(|h'|, 1e-10, 1 - 1e-5)    arsech(x) = log((1 + sqrt(1 - x^2)) / x): the reference's log map
//   u_w = u_e o wu[r]
//   u_m = (1 / cosh(n)) u_w / n,  n = max(|u_w|, 1e-10)          1 / cosh: the reference's exponential map
//   v_m = p_sum(t', r');  u_m, v_m clipped
//   preds = -((2 arsech(clamp(|p_sum(-u_m, v_m)|, 1e-10, 1 - 1e-5)))^2 - bs[h] - bo[t])
//
// Neither map is the Poincare ball's (artanh, tanh); they are the maps the reference's checkpoints were trained with and are kept.
//
// One lane group (16 lanes up to 48 columns, else 64) holds a triple: its rows sit in registers (zero past the last column) and every
// k-long reduction is a cross-lane butterfly, so all lanes of a group hold the same scalars bit for bit and branch together.  The
// backward is hand-derived with autograd's conventions: `where` passes the chosen branch's gradient only, clamp passes it on the
// closed interval, the 2-norm has gradient 0 at 0, rows 0 of the two embeddings get nothing (padding_idx = 0), index 0 of wu / bs / bo
// does.  A saturated last clamp ends the backward after bs / bo: wu, ent and rel receive nothing, exactly as autograd's zeros.
// Gradients are scattered with float64 global atomic adds (native on gfx950): sums are not bit-reproducible run to run.
//
// k_murp_rsgd is the optimiser in one launch: the Poincare update (riemannian_optimizer.py) on the rows of the two embeddings,
// p -= lr g on wu, bs, bo; it clears the gradients it reads and leaves rows (elements) with a zero gradient unwritten.
//
// The rank sweep contracts a (query, candidate) pair to two dot products and the candidate's squared norm; the rest of the score is
// scalar work per pair (murp_pair).  The true candidate's score and the filter lists' are computed with the same accumulation order as
// the sweep's, so equal scores are equal bit for bit and the counts are exact with respect to the stored scores.
#include <math.h>
#include "kge_internal.h"
#include "kge_projection.h"   // ws_check

namespace kge {
namespace {

constexpr int kMuBlock = 256;
constexpr int kMuMaxBlocks = 256 * 8;
constexpr double kMuBall = 1.0 - 1e-5;    // the clamps' upper bound
constexpr double kMuEps = 1e-5;           // the clips divide by |x| - kMuEps
constexpr double kMuTiny = 1e-10;

struct MuArgs {
    const double *wu, *bs, *bo, *ent, *rel;
    double *g_wu, *g_bs, *g_bo, *g_ent, *g_rel;
    int k;
};

template <int G>
__device__ __forceinline__ double gsumd(double v) {
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}
template <int G, int N>
__device__ __forceinline__ double vdot(const double (&a)[N], const double (&b)[N]) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) s += a[c] * b[c];
    return gsumd<G>(s);
}
template <int G, int N>
__device__ __forceinline__ void load_rowd(double (&x)[N], const double* __restrict__ row, int k, int gl) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int e = c * G + gl;
        x[c] = e < k ? row[e] : 0.0;
    }
}
template <int G, int N>
__device__ __forceinline__ void atomic_add_rowd(double* __restrict__ row, const double (&g)[N], int k, int gl) {
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int e = c * G + gl;
        if (e < k) unsafeAtomicAdd(row + e, g[c]);   // global_atomic_add_f64
    }
}

__device__ __forceinline__ double mu_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ bool mu_inside(double x, double lo, double hi) { return x >= lo && x <= hi; }
__device__ __forceinline__ double mu_arsech(double x) { return log((1.0 + sqrt(1.0 - x * x)) / x); }
__device__ __forceinline__ double mu_d_arsech(double x) { return -1.0 / (x * sqrt(1.0 - x * x)); }

// out = clip(x); n = |x|; returns whether the row was outside the ball
template <int G, int N>
__device__ __forceinline__ bool clip_fwd(const double (&x)[N], double (&out)[N], double& n) {
    n = sqrt(vdot<G, N>(x, x));
    const bool m = n >= 1.0;
    const double d = n - kMuEps;
#pragma unroll
    for (int c = 0; c < N; ++c) out[c] = m ? x[c] / d : x[c];
    return m;
}
// g (gradient of the clipped row) -> gradient of x, in place
template <int G, int N>
__device__ __forceinline__ void clip_bwd(const double (&x)[N], double n, bool m, double (&g)[N]) {
    if (!m) return;
    const double d = n - kMuEps;
    const double s = vdot<G, N>(g, x) / (d * d * n);
#pragma unroll
    for (int c = 0; c < N; ++c) g[c] = g[c] / d - s * x[c];
}

struct PSum { double sxr, syr, sx, sy, A, B, den; };
template <int G, int N>
__device__ __forceinline__ void psum_fwd(const double (&x)[N], const double (&y)[N], double (&out)[N], PSum& s) {
    s.sxr = vdot<G, N>(x, x);
    s.syr = vdot<G, N>(y, y);
    const double dxy = vdot<G, N>(x, y);
    s.sx = mu_clamp(s.sxr, 0.0, kMuBall);
    s.sy = mu_clamp(s.syr, 0.0, kMuBall);
    s.A = 1.0 + 2.0 * dxy + s.sy;
    s.B = 1.0 - s.sx;
    s.den = 1.0 + 2.0 * dxy + s.sx * s.sy;
#pragma unroll
    for (int c = 0; c < N; ++c) out[c] = (s.A * x[c] + s.B * y[c]) / s.den;
}
// g = gradient of out -> gx, gy
template <int G, int N>
__device__ __forceinline__ void psum_bwd(const double (&x)[N], const double (&y)[N], const double (&out)[N], const PSum& s,
                                         const double (&g)[N], double (&gx)[N], double (&gy)[N]) {
    const double g_den = -vdot<G, N>(g, out) / s.den;
    const double gA = vdot<G, N>(g, x) / s.den;
    const double gB = vdot<G, N>(g, y) / s.den;
    const double g_dxy = 2.0 * gA + 2.0 * g_den;
    const double g_sy = mu_inside(s.syr, 0.0, kMuBall) ? gA + g_den * s.sx : 0.0;
    const double g_sx = mu_inside(s.sxr, 0.0, kMuBall) ? -gB + g_den * s.sy : 0.0;
    const double ca = s.A / s.den, cb = s.B / s.den;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        gx[c] = ca * g[c] + g_dxy * y[c] + 2.0 * g_sx * x[c];
        gy[c] = cb * g[c] + g_dxy * x[c] + 2.0 * g_sy * y[c];
    }
}

// One lane group per triple.  BWD = false: preds[i].  BWD = true: the gradients of sum_i dscore[i] preds_i (dscore given) or of
// mean_i BCE-with-logits(preds_i, clamp(y_i, 0, 1)) with the loss added to *loss (y given).
template <int G, int N, bool BWD>
__global__ __launch_bounds__(kMuBlock) void k_murp_rows(MuArgs a, const int64_t* __restrict__ h, const int64_t* __restrict__ r,
                                                        const int64_t* __restrict__ t, const int64_t* __restrict__ y,
                                                        const double* __restrict__ dscore, int64_t n, double* __restrict__ preds,
                                                        double* __restrict__ loss) {
    const int gl = threadIdx.x % G;
    const int64_t groups = (int64_t)gridDim.x * (kMuBlock / G);
    double lacc = 0.0;
    for (int64_t i = ((int64_t)blockIdx.x * kMuBlock + threadIdx.x) / G; i < n; i += groups) {
        const int64_t ih = h[i], ir = r[i], it = t[i];
        double eh[N], et[N], er[N], w[N];
        load_rowd<G, N>(eh, a.ent + ih * a.k, a.k, gl);
        load_rowd<G, N>(et, a.ent + it * a.k, a.k, gl);
        load_rowd<G, N>(er, a.rel + ir * a.k, a.k, gl);
        load_rowd<G, N>(w, a.wu + ir * a.k, a.k, gl);
        double hc[N], tc[N], rc[N], nh, nt, nr;
        const bool mh = clip_fwd<G, N>(eh, hc, nh);
        const bool mt = clip_fwd<G, N>(et, tc, nt);
        const bool mr = clip_fwd<G, N>(er, rc, nr);
        // log map, the relation's diagonal, exponential map
        const double nh1 = sqrt(vdot<G, N>(hc, hc));
        const double cc = mu_clamp(nh1, kMuTiny, kMuBall);
        const double ac = mu_arsech(cc);
        double ue[N], uw[N], um[N];
#pragma unroll
        for (int c = 0; c < N; ++c) {
            ue[c] = ac * hc[c] / cc;
            uw[c] = ue[c] * w[c];
        }
        const double nwr = sqrt(vdot<G, N>(uw, uw));
        const double nw = nwr < kMuTiny ? kMuTiny : nwr;
        const double ich = 1.0 / cosh(nw);
#pragma unroll
        for (int c = 0; c < N; ++c) um[c] = ich * uw[c] / nw;
        double vm[N], umc[N], vmc[N], z[N], num, nvm;
        PSum ps1, ps2;
        psum_fwd<G, N>(tc, rc, vm, ps1);
        const bool mu = clip_fwd<G, N>(um, umc, num);
        const bool mv = clip_fwd<G, N>(vm, vmc, nvm);
        double xn[N];
#pragma unroll
        for (int c = 0; c < N; ++c) xn[c] = -umc[c];
        psum_fwd<G, N>(xn, vmc, z, ps2);
        const double nz = sqrt(vdot<G, N>(z, z));
        const double cz = mu_clamp(nz, kMuTiny, kMuBall);
        const double az = mu_arsech(cz);
        const double two_az = 2.0 * az;
        const double score = -(two_az * two_az - a.bs[ih] - a.bo[it]);
        if constexpr (!BWD) {
            if (gl == 0) preds[i] = score;
        } else {
            double gs;
            if (dscore) {
                gs = dscore[i];
            } else {   // BCEWithLogitsLoss()(preds, clamp(y, 0, 1)): the mean over the n rows
                const double lab = y[i] >= 1 ? 1.0 : 0.0;
                const double ex = exp(-fabs(score));
                if (gl == 0) lacc += ((score > 0.0 ? score : 0.0) - score * lab + log1p(ex)) / (double)n;
                gs = ((score >= 0.0 ? 1.0 / (1.0 + ex) : ex / (1.0 + ex)) - lab) / (double)n;
            }
            if (gl == 0) {
                unsafeAtomicAdd(a.g_bs + ih, gs);
                unsafeAtomicAdd(a.g_bo + it, gs);
            }
            // score = -(sq - bs - bo), sq = (2 arsech(cz))^2, cz = clamp(|z|)
            const double g_nz = mu_inside(nz, kMuTiny, kMuBall) ? -gs * 8.0 * az * mu_d_arsech(cz) : 0.0;
            if (g_nz == 0.0 || !(nz > 0.0)) continue;   // a saturated clamp (or gs = 0): nothing reaches wu, ent, rel
            double gz[N], gx[N], gvm[N];
#pragma unroll
            for (int c = 0; c < N; ++c) gz[c] = g_nz * z[c] / nz;
            psum_bwd<G, N>(xn, vmc, z, ps2, gz, gx, gvm);
            double gum[N];
#pragma unroll
            for (int c = 0; c < N; ++c) gum[c] = -gx[c];
            clip_bwd<G, N>(um, num, mu, gum);
            clip_bwd<G, N>(vm, nvm, mv, gvm);
            double gt[N], gr[N];
            psum_bwd<G, N>(tc, rc, vm, ps1, gvm, gt, gr);
            clip_bwd<G, N>(et, nt, mt, gt);
            clip_bwd<G, N>(er, nr, mr, gr);
            if (it != 0) atomic_add_rowd<G, N>(a.g_ent + it * a.k, gt, a.k, gl);
            if (ir != 0) atomic_add_rowd<G, N>(a.g_rel + ir * a.k, gr, a.k, gl);
            // u_m = (1 / cosh(nw)) u_w / nw, nw = max(|u_w|, 1e-10)
            const double gf = ich / nw;
            const double d_gf = -(tanh(nw) * nw + 1.0) * ich / (nw * nw);
            const double g_nw = nwr >= kMuTiny ? vdot<G, N>(gum, uw) * d_gf : 0.0;
            double gw[N], gh[N];
#pragma unroll
            for (int c = 0; c < N; ++c) {
                const double guw = gf * gum[c] + (nwr > 0.0 ? g_nw * uw[c] / nwr : 0.0);
                gw[c] = guw * ue[c];
                gh[c] = guw * w[c];    // gradient of u_e
            }
            atomic_add_rowd<G, N>(a.g_wu + ir * a.k, gw, a.k, gl);
            // u_e = arsech(c) h' / c, c = clamp(|h'|)
            const double d_f = (mu_d_arsech(cc) * cc - ac) / (cc * cc);
            const double g_c = mu_inside(nh1, kMuTiny, kMuBall) ? vdot<G, N>(gh, hc) * d_f : 0.0;
            const double fh = ac / cc;
#pragma unroll
            for (int c = 0; c < N; ++c) gh[c] = fh * gh[c] + (nh1 > 0.0 ? g_c * hc[c] / nh1 : 0.0);
            clip_bwd<G, N>(eh, nh, mh, gh);
            if (ih != 0) atomic_add_rowd<G, N>(a.g_ent + ih * a.k, gh, a.k, gl);
        }
    }
    if constexpr (BWD) {
        if (loss) {   // (all lanes are back together here: one atomic per wave)
            lacc = gsumd<64>(lacc);
            if ((threadIdx.x & 63) == 0 && lacc != 0.0) unsafeAtomicAdd(loss, lacc);
        }
    }
}

// The optimiser.  Blocks [0, row_blocks): one lane group per row of ent then rel, the Poincare update in the reference's operation
// order.  The other blocks: p -= lr g over the elements of wu | bs | bo (| ent | rel when there are no row blocks).
template <int G, int N>
__global__ __launch_bounds__(kMuBlock) void k_murp_rsgd(MuArgs a, int64_t E, int64_t R, double lr, unsigned row_blocks) {
    if (blockIdx.x < row_blocks) {
        const int gl = threadIdx.x % G;
        const int64_t groups = (int64_t)row_blocks * (kMuBlock / G);
        for (int64_t i = ((int64_t)blockIdx.x * kMuBlock + threadIdx.x) / G; i < E + R; i += groups) {
            double* prow = (i < E ? const_cast<double*>(a.ent) + i * a.k : const_cast<double*>(a.rel) + (i - E) * a.k);
            double* grow = (i < E ? a.g_ent + i * a.k : a.g_rel + (i - E) * a.k);
            double d[N];
            load_rowd<G, N>(d, grow, a.k, gl);
            double any = 0.0;
#pragma unroll
            for (int c = 0; c < N; ++c) any += d[c] != 0.0 ? 1.0 : 0.0;
            if (gsumd<G>(any) == 0.0) continue;    // p_sum(p, 0) = p exactly: the row is left unwritten
            double p[N], v[N], yv[N], out[N];
            load_rowd<G, N>(p, prow, a.k, gl);
            const double sq = mu_clamp(vdot<G, N>(p, p), 0.0, kMuBall);
            const double scale = (1.0 - sq) * (1.0 - sq) / 4.0;
#pragma unroll
            for (int c = 0; c < N; ++c) v[c] = -lr * (d[c] * scale);
            const double nvr = sqrt(vdot<G, N>(v, v));
            const double nv = nvr < kMuTiny ? kMuTiny : nvr;
            const double th = tanh(nv / (1.0 - sq));
#pragma unroll
            for (int c = 0; c < N; ++c) yv[c] = th * v[c] / nv;
            PSum s;
            psum_fwd<G, N>(p, yv, out, s);
#pragma unroll
            for (int c = 0; c < N; ++c) {
                const int e = c * G + gl;
                if (e < a.k) { prow[e] = out[c]; grow[e] = 0.0; }
            }
        }
        return;
    }
    const int64_t n_wu = R * a.k;
    const int64_t n_flat = n_wu + 2 * E;
    const int64_t total = n_flat + (row_blocks ? 0 : (E + R) * a.k);
    const int64_t stride = (int64_t)(gridDim.x - row_blocks) * kMuBlock;
    for (int64_t i = (int64_t)(blockIdx.x - row_blocks) * kMuBlock + threadIdx.x; i < total; i += stride) {
        double *p, *g;
        if (i < n_wu) { p = const_cast<double*>(a.wu) + i; g = a.g_wu + i; }
        else if (i < n_wu + E) { p = const_cast<double*>(a.bs) + (i - n_wu); g = a.g_bs + (i - n_wu); }
        else if (i < n_flat) { p = const_cast<double*>(a.bo) + (i - n_wu - E); g = a.g_bo + (i - n_wu - E); }
        else if (i < n_flat + E * a.k) { p = const_cast<double*>(a.ent) + (i - n_flat); g = a.g_ent + (i - n_flat); }
        else { p = const_cast<double*>(a.rel) + (i - n_flat - E * a.k); g = a.g_rel + (i - n_flat - E * a.k); }
        const double gv = *g;
        if (gv != 0.0) { *p = *p - lr * gv; *g = 0.0; }
    }
}

// ---------------------------------------------------------------- rank sweep
// Per query: two vectors q1, q2 [k] and four scalars.
//   tail sweep of (h, r): q1 = r', q2 = u_m (finished);      scalars |u_m|^2, |r'|^2, r'.u_m, bs[h]
//   head sweep of (r, t): q1 = wu o wu, q2 = wu o v_m;       scalars |v_m|^2, -, -, bo[t]          (v_m finished)
// Per pair: d1 = sum f(e_j) q1_j (f(e) = e for the tail sweep, e^2 for the head sweep), d2 = sum e_j q2_j, ne2 = sum e_j^2, each
// accumulated in column order from 0.
struct MuEval {
    double* qv;        // [nq, 2, k]
    double* qs;        // [nq, 4]
    double* st;        // [nq] the true candidate's score
    int* cnt;          // [nq, 2] candidates before the true one, candidates equal to it (itself included)
    int64_t nq;
    int side;          // 0 / 1: every query is that side's; 2: query j is triple j >> 1, head sweep when j is odd
};
__device__ __forceinline__ bool mu_head(const MuEval& ev, int64_t q) { return ev.side == 2 ? (q & 1) != 0 : ev.side == 1; }
__device__ __forceinline__ int64_t mu_triple(const MuEval& ev, int64_t q) { return ev.side == 2 ? q >> 1 : q; }

template <int G, int N>
__global__ __launch_bounds__(kMuBlock) void k_murp_query(MuArgs a, MuEval ev, const int64_t* __restrict__ triples) {
    const int gl = threadIdx.x % G;
    const int64_t groups = (int64_t)gridDim.x * (kMuBlock / G);
    for (int64_t q = ((int64_t)blockIdx.x * kMuBlock + threadIdx.x) / G; q < ev.nq; q += groups) {
        const int64_t* trip = triples + 3 * mu_triple(ev, q);
        const int64_t ih = trip[0], ir = trip[1], it = trip[2];
        const bool head = mu_head(ev, q);
        double w[N], er[N], rc[N], nr;
        load_rowd<G, N>(w, a.wu + ir * a.k, a.k, gl);
        load_rowd<G, N>(er, a.rel + ir * a.k, a.k, gl);
        clip_fwd<G, N>(er, rc, nr);
        double q1[N], q2[N], s0, s1 = 0.0, s2 = 0.0, s3;
        if (!head) {
            double eh[N], hc[N], nh, um[N], num;
            load_rowd<G, N>(eh, a.ent + ih * a.k, a.k, gl);
            clip_fwd<G, N>(eh, hc, nh);
            const double cc = mu_clamp(sqrt(vdot<G, N>(hc, hc)), kMuTiny, kMuBall);
            const double ac = mu_arsech(cc);
#pragma unroll
            for (int c = 0; c < N; ++c) um[c] = (ac * hc[c] / cc) * w[c];
            const double nwr = sqrt(vdot<G, N>(um, um));
            const double nw = nwr < kMuTiny ? kMuTiny : nwr;
            const double ich = 1.0 / cosh(nw);
#pragma unroll
            for (int c = 0; c < N; ++c) um[c] = ich * um[c] / nw;
            clip_fwd<G, N>(um, q2, num);
#pragma unroll
            for (int c = 0; c < N; ++c) q1[c] = rc[c];
            s0 = vdot<G, N>(q2, q2); s1 = vdot<G, N>(rc, rc); s2 = vdot<G, N>(rc, q2); s3 = a.bs[ih];
        } else {
            double et[N], tc[N], nt, vm[N], vmc[N], nvm;
            PSum ps;
            load_rowd<G, N>(et, a.ent + it * a.k, a.k, gl);
            clip_fwd<G, N>(et, tc, nt);
            psum_fwd<G, N>(tc, rc, vm, ps);
            clip_fwd<G, N>(vm, vmc, nvm);
#pragma unroll
            for (int c = 0; c < N; ++c) { q1[c] = w[c] * w[c]; q2[c] = w[c] * vmc[c]; }
            s0 = vdot<G, N>(vmc, vmc); s3 = a.bo[it];
        }
        double* qv = ev.qv + q * 2 * a.k;
#pragma unroll
        for (int c = 0; c < N; ++c) {
            const int e = c * G + gl;
            if (e < a.k) { qv[e] = q1[c]; qv[a.k + e] = q2[c]; }
        }
        if (gl == 0) { double* qs = ev.qs + 4 * q; qs[0] = s0; qs[1] = s1; qs[2] = s2; qs[3] = s3; }
    }
}

// (factor, clipped squared norm) of a vector with squared norm n2
__device__ __forceinline__ double mu_clip_factor(double n2, double& clipped) {
    const double n = sqrt(n2);
    const double f = n >= 1.0 ? 1.0 / (n - kMuEps) : 1.0;
    clipped = f * f * n2;
    return f;
}
// preds of the pair from its three sums (the formulas: DESIGN.md section 24, tools/murp_reference.py sweep_tail / sweep_head)
__device__ __forceinline__ double murp_pair(bool head, double d1, double d2, double ne2, const double* __restrict__ qs, double bs_e,
                                            double bo_e) {
    double su, sv, duv;     // |u_m|^2, |v_m|^2, u_m . v_m, all finished (clipped)
    double se;
    const double ce = mu_clip_factor(ne2, se);
    if (!head) {
        const double sr = qs[1], dru = qs[2];
        const double dtr = ce * d1, dtu = ce * d2;
        const double sx = mu_clamp(se, 0.0, kMuBall), sy = mu_clamp(sr, 0.0, kMuBall);
        const double A = 1.0 + 2.0 * dtr + sy, B = 1.0 - sx, den = 1.0 + 2.0 * dtr + sx * sy;
        const double svr = (A * A * se + 2.0 * A * B * dtr + B * B * sr) / (den * den);
        const double cv = mu_clip_factor(svr, sv);
        duv = cv * ((A * dtu + B * dru) / den);
        su = qs[0];
    } else {
        const double cc = mu_clamp(sqrt(se), kMuTiny, kMuBall);
        const double f = mu_arsech(cc) / cc * ce;         // u_w = f (e o wu)
        const double sw = f * f * d1;
        const double nwr = sqrt(sw);
        const double nw = nwr < kMuTiny ? kMuTiny : nwr;
        const double gf = (1.0 / cosh(nw)) / nw;
        const double cu = mu_clip_factor(gf * gf * sw, su);
        duv = cu * (gf * f * d2);
        sv = qs[0];
    }
    // |p_sum(-u, v)|^2
    const double sx = mu_clamp(su, 0.0, kMuBall), sy = mu_clamp(sv, 0.0, kMuBall);
    const double A = 1.0 - 2.0 * duv + sy, B = 1.0 - sx, den = 1.0 - 2.0 * duv + sx * sy;
    const double nz2 = (A * A * su - 2.0 * A * B * duv + B * B * sv) / (den * den);
    const double cz = mu_clamp(sqrt(nz2 > 0.0 ? nz2 : 0.0), kMuTiny, kMuBall);
    const double two_az = 2.0 * mu_arsech(cz);
    return head ? -(two_az * two_az - bs_e - qs[3]) : -(two_az * two_az - qs[3] - bo_e);
}
// the pair (query q, candidate e) with its sums taken serially: the order of the sweep's accumulation
__device__ __forceinline__ double murp_pair_serial(const MuArgs& a, const MuEval& ev, int64_t q, int64_t e) {
    const bool head = mu_head(ev, q);
    const double* row = a.ent + e * a.k;
    const double* q1 = ev.qv + q * 2 * a.k;
    const double* q2 = q1 + a.k;
    double d1 = 0.0, d2 = 0.0, ne2 = 0.0;
    for (int j = 0; j < a.k; ++j) {
        const double x = row[j];
        d1 += (head ? x * x : x) * q1[j];
        d2 += x * q2[j];
        ne2 += x * x;
    }
    return murp_pair(head, d1, d2, ne2, ev.qs + 4 * q, a.bs[e], a.bo[e]);
}
__device__ __forceinline__ bool mu_before(int rank_order, double s, double st) { return rank_order ? s > st : s < st; }

__global__ __launch_bounds__(kMuBlock) void k_murp_truth(MuArgs a, MuEval ev, const int64_t* __restrict__ triples) {
    const int64_t q = (int64_t)blockIdx.x * kMuBlock + threadIdx.x;
    if (q >= ev.nq) return;
    const int64_t tr = triples[3 * mu_triple(ev, q) + (mu_head(ev, q) ? 0 : 2)];
    ev.st[q] = murp_pair_serial(a, ev, q, tr);
}

constexpr int kMuTileE = 64;     // candidates of a tile: one per lane
constexpr int kMuTileK = 32;     // columns of a chunk
constexpr int kMuQPT = 4;        // queries per thread
constexpr int kMuTileQ = (kMuBlock / kMuTileE) * kMuQPT;   // 16 queries per workgroup

// grid (candidate tiles, query tiles).  scores != NULL: scores[q, e]; else counts against ev.st into ev.cnt.
__global__ __launch_bounds__(kMuBlock) void k_murp_sweep(MuArgs a, MuEval ev, int64_t E, int rank_order, double* __restrict__ scores) {
    __shared__ double cand[kMuTileE][kMuTileK + 1];
    __shared__ double qch[kMuTileQ][2][kMuTileK];
    const int lane = threadIdx.x & 63, slot = threadIdx.x >> 6;
    const int64_t e0 = (int64_t)blockIdx.x * kMuTileE, q0 = (int64_t)blockIdx.y * kMuTileQ + slot * kMuQPT;
    double d1[kMuQPT], d2[kMuQPT], ne2 = 0.0;
    bool head[kMuQPT];
#pragma unroll
    for (int j = 0; j < kMuQPT; ++j) { d1[j] = 0.0; d2[j] = 0.0; head[j] = mu_head(ev, q0 + j); }
    for (int kc = 0; kc < a.k; kc += kMuTileK) {
        __syncthreads();
        for (int i = threadIdx.x; i < kMuTileE * kMuTileK; i += kMuBlock) {
            const int row = i / kMuTileK, col = i % kMuTileK;
            cand[row][col] = (e0 + row < E && kc + col < a.k) ? a.ent[(e0 + row) * a.k + kc + col] : 0.0;
        }
        for (int i = threadIdx.x; i < kMuTileQ * 2 * kMuTileK; i += kMuBlock) {
            const int col = i % kMuTileK, v = (i / kMuTileK) & 1, qi = i / (2 * kMuTileK);
            const int64_t q = (int64_t)blockIdx.y * kMuTileQ + qi;
            qch[qi][v][col] = (q < ev.nq && kc + col < a.k) ? ev.qv[(q * 2 + v) * a.k + kc + col] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int c = 0; c < kMuTileK; ++c) {
            const double x = cand[lane][c];
            const double xx = x * x;
            ne2 += xx;
#pragma unroll
            for (int j = 0; j < kMuQPT; ++j) {
                d1[j] += (head[j] ? xx : x) * qch[slot * kMuQPT + j][0][c];
                d2[j] += x * qch[slot * kMuQPT + j][1][c];
            }
        }
    }
    const int64_t e = e0 + lane;
    const double bs_e = e < E ? a.bs[e] : 0.0, bo_e = e < E ? a.bo[e] : 0.0;
#pragma unroll
    for (int j = 0; j < kMuQPT; ++j) {
        const int64_t q = q0 + j;
        if (q >= ev.nq) break;    // (wave-uniform: q depends on the wave's slot only)
        const bool live = e < E;
        const double s = live ? murp_pair(head[j], d1[j], d2[j], ne2, ev.qs + 4 * q, bs_e, bo_e) : 0.0;
        if (scores) {
            if (live) scores[q * E + e] = s;
        } else {
            const double st = ev.st[q];
            const int nb = __popcll(__ballot(live && mu_before(rank_order, s, st)));
            const int ne = __popcll(__ballot(live && s == st));
            if (lane == 0) {
                if (nb) atomicAdd(ev.cnt + 2 * q, nb);
                if (ne) atomicAdd(ev.cnt + 2 * q + 1, ne);
            }
        }
    }
}

// one wave per query: the filter list's candidates that come before the true one, then the query's four numbers
__global__ __launch_bounds__(kMuBlock) void k_murp_finish(MuArgs a, MuEval ev, const int64_t* __restrict__ triples, int64_t n, int rank_order,
                                                          const int64_t* __restrict__ tail_off, const int32_t* __restrict__ tail_ids,
                                                          const int64_t* __restrict__ head_off, const int32_t* __restrict__ head_ids,
                                                          int32_t* __restrict__ ranks, int32_t* __restrict__ ties) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (kMuBlock / 64) + (threadIdx.x >> 6);
    if (q >= ev.nq) return;
    const int64_t i = mu_triple(ev, q);
    const bool head = mu_head(ev, q);
    const int64_t tr = triples[3 * i + (head ? 0 : 2)];
    const double st = ev.st[q];
    const int64_t* off = head ? head_off : tail_off;
    const int32_t* ids = head ? head_ids : tail_ids;
    int fc = 0;
    if (off) {
        for (int64_t j = off[i] + lane; j < off[i + 1]; j += 64) {
            const int64_t e = ids[j];
            if (e != tr && mu_before(rank_order, murp_pair_serial(a, ev, q, e), st)) ++fc;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) fc += __shfl_xor(fc, o, 64);
    if (lane == 0) {
        const int cnt = ev.cnt[2 * q];
        ranks[(head ? 0 : 1) * n + i] = cnt;
        ranks[(head ? 2 : 3) * n + i] = cnt - fc;
        if (ties) ties[(head ? 0 : 1) * n + i] = ev.cnt[2 * q + 1] - 1;
    }
}

// ---------------------------------------------------------------- host side
int mu_check(const kge_murp_desc* d, const char* who, bool grads) {
    if (!d) { set_error("%s: null descriptor", who); return -1; }
    for (int i = 0; i < 5; ++i)
        if (!d->tables[i]) { set_error("%s: null tables (wu, bs, bo, ent and rel are all required)", who); return -1; }
    if (d->tot_entity < 1 || d->tot_relation < 1) {
        set_error("%s: tot_entity and tot_relation must be positive (got %lld, %lld)", who, (long long)d->tot_entity, (long long)d->tot_relation);
        return -1;
    }
    if (d->dim < 1 || d->dim > 2048) { set_error("%s: dim must be 1..2048 (got %d)", who, d->dim); return -1; }
    if (d->rank_order != 0 && d->rank_order != 1) {
        set_error("%s: rank_order is 0 (ascending score, the reference's lists) or 1 (most plausible first), got %d", who, d->rank_order);
        return -1;
    }
    if (grads)
        for (int i = 0; i < 5; ++i)
            if (!d->grads[i]) { set_error("%s: null gradient buffers (all five are required)", who); return -1; }
    return 0;
}

MuArgs mu_args(const kge_murp_desc* d) {
    return MuArgs{d->tables[0], d->tables[1], d->tables[2], d->tables[3], d->tables[4],
                  d->grads[0], d->grads[1], d->grads[2], d->grads[3], d->grads[4], d->dim};
}

kge_model_desc mu_id_bounds(const kge_murp_desc* d) {   // what the id scans of the debug mode read
    kge_model_desc m{};
    m.tot_entity = d->tot_entity; m.tot_relation = d->tot_relation;
    return m;
}

// the lane group and the columns a lane holds: (16, 1) (16, 3) (64, 2) (64, 8) (64, 32)
#define MU_DISPATCH(k, CALL)                          \
    do {                                              \
        if ((k) <= 16) { CALL(16, 1); }               \
        else if ((k) <= 48) { CALL(16, 3); }          \
        else if ((k) <= 128) { CALL(64, 2); }         \
        else if ((k) <= 512) { CALL(64, 8); }         \
        else { CALL(64, 32); }                        \
    } while (0)
int mu_group(int k) { return k <= 48 ? 16 : 64; }
unsigned mu_row_blocks(int k, int64_t rows) {
    const int gpb = kMuBlock / mu_group(k);
    int64_t b = (rows + gpb - 1) / gpb;
    if (b > kMuMaxBlocks) b = kMuMaxBlocks;
    return (unsigned)(b < 1 ? 1 : b);
}

int mu_rows(const kge_murp_desc* d, bool bwd, const int64_t* h, const int64_t* r, const int64_t* t, const int64_t* y, const double* dscore,
            int64_t n, double* preds, double* loss, hipStream_t s) {
    const MuArgs a = mu_args(d);
    const dim3 grid(mu_row_blocks(d->dim, n)), block(kMuBlock);
#define MU_ROWS(G, N)                                                                                                       \
    if (bwd) hipLaunchKernelGGL((k_murp_rows<G, N, true>), grid, block, 0, s, a, h, r, t, y, dscore, n, preds, loss);        \
    else hipLaunchKernelGGL((k_murp_rows<G, N, false>), grid, block, 0, s, a, h, r, t, y, dscore, n, preds, loss)
    MU_DISPATCH(d->dim, MU_ROWS);
#undef MU_ROWS
    return check_launch("k_murp_rows");
}

struct MuEvalPlan { size_t qv, qs, st, cnt, total; };
MuEvalPlan mu_eval_plan(const kge_murp_desc* d, int64_t nq) {
    MuEvalPlan p;
    p.qv = 0;
    p.qs = p.qv + align256((size_t)nq * 2 * (size_t)d->dim * sizeof(double));
    p.st = p.qs + align256((size_t)nq * 4 * sizeof(double));
    p.cnt = p.st + align256((size_t)nq * sizeof(double));
    p.total = p.cnt + align256((size_t)nq * 2 * sizeof(int));
    return p;
}
MuEval mu_eval(const kge_murp_desc* d, void* ws, int64_t nq, int side) {
    const MuEvalPlan p = mu_eval_plan(d, nq);
    char* b = (char*)ws;
    return MuEval{(double*)(b + p.qv), (double*)(b + p.qs), (double*)(b + p.st), (int*)(b + p.cnt), nq, side};
}
int mu_queries(const kge_murp_desc* d, const MuEval& ev, const int64_t* triples, hipStream_t s) {
    const MuArgs a = mu_args(d);
    const dim3 grid(mu_row_blocks(d->dim, ev.nq)), block(kMuBlock);
#define MU_QUERY(G, N) hipLaunchKernelGGL((k_murp_query<G, N>), grid, block, 0, s, a, ev, triples)
    MU_DISPATCH(d->dim, MU_QUERY);
#undef MU_QUERY
    return check_launch("k_murp_query");
}
// grid.y is limited to 65535 query tiles: longer query lists go in slices
int mu_sweep(const kge_murp_desc* d, MuEval ev, double* scores, hipStream_t s) {
    const MuArgs a = mu_args(d);
    const int64_t E = d->tot_entity;
    const int64_t per = (int64_t)32768 * kMuTileQ;   // (even: the two sides of a triple stay interleaved)
    for (int64_t q0 = 0; q0 < ev.nq; q0 += per) {
        MuEval part = ev;
        part.nq = ev.nq - q0 < per ? ev.nq - q0 : per;
        part.qv += q0 * 2 * d->dim; part.qs += 4 * q0; part.st += q0; part.cnt += 2 * q0;
        const dim3 grid((unsigned)((E + kMuTileE - 1) / kMuTileE), (unsigned)((part.nq + kMuTileQ - 1) / kMuTileQ));
        hipLaunchKernelGGL(k_murp_sweep, grid, dim3(kMuBlock), 0, s, a, part, E, d->rank_order, scores ? scores + q0 * E : nullptr);
    }
    return check_launch("k_murp_sweep");
}

}  // namespace
}  // namespace kge

using namespace kge;

extern "C" {

int kge_murp_score_forward(const kge_murp_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n, double* preds,
                           void* stream) {
    const char* who = "kge_murp_score_forward";
    if (mu_check(d, who, false)) return -1;
    if (n < 0 || (n > 0 && (!h || !r || !t || !preds))) { set_error("%s: bad arguments", who); return -1; }
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const kge_model_desc bounds = mu_id_bounds(d);
    if (int rc = debug_check_hrt(who, &bounds, h, r, t, n, s)) return rc;
    return mu_rows(d, false, h, r, t, nullptr, nullptr, n, preds, nullptr, s);
}

int kge_murp_score_backward(const kge_murp_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n, const double* dscore,
                            void* stream) {
    const char* who = "kge_murp_score_backward";
    if (mu_check(d, who, true)) return -1;
    if (n < 0 || (n > 0 && (!h || !r || !t || !dscore))) { set_error("%s: bad arguments", who); return -1; }
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const kge_model_desc bounds = mu_id_bounds(d);
    if (int rc = debug_check_hrt(who, &bounds, h, r, t, n, s)) return rc;
    return mu_rows(d, true, h, r, t, nullptr, dscore, n, nullptr, nullptr, s);
}

int kge_murp_train_bce(const kge_murp_desc* d, const int64_t* h, const int64_t* r, const int64_t* t, const int64_t* y, int64_t n,
                       double* loss, void* stream) {
    const char* who = "kge_murp_train_bce";
    if (mu_check(d, who, true)) return -1;
    if (n < 0 || !loss || (n > 0 && (!h || !r || !t || !y))) { set_error("%s: bad arguments", who); return -1; }
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const kge_model_desc bounds = mu_id_bounds(d);
    if (int rc = debug_check_hrt(who, &bounds, h, r, t, n, s)) return rc;
    return mu_rows(d, true, h, r, t, y, nullptr, n, nullptr, loss, s);
}

int kge_murp_rsgd_step(const kge_murp_desc* d, double lr, int32_t riemannian, void* stream) {
    const char* who = "kge_murp_rsgd_step";
    if (mu_check(d, who, true)) return -1;
    const MuArgs a = mu_args(d);
    const int64_t E = d->tot_entity, R = d->tot_relation;
    const unsigned row_blocks = riemannian ? mu_row_blocks(d->dim, E + R) : 0u;
    const int64_t flat = R * d->dim + 2 * E + (riemannian ? 0 : (E + R) * (int64_t)d->dim);
    int64_t fb = (flat + kMuBlock - 1) / kMuBlock;
    if (fb > kMuMaxBlocks) fb = kMuMaxBlocks;
    const dim3 grid(row_blocks + (unsigned)fb), block(kMuBlock);
    hipStream_t s = (hipStream_t)stream;
#define MU_RSGD(G, N) hipLaunchKernelGGL((k_murp_rsgd<G, N>), grid, block, 0, s, a, E, R, lr, row_blocks)
    MU_DISPATCH(d->dim, MU_RSGD);
#undef MU_RSGD
    return check_launch("k_murp_rsgd");
}

size_t kge_murp_eval_ranks_workspace_bytes(const kge_murp_desc* d, int64_t n) {
    if (mu_check(d, "kge_murp_eval_ranks_workspace_bytes", false) || n < 0) return 0;
    return mu_eval_plan(d, 2 * (n > 0 ? n : 1)).total;
}

size_t kge_murp_sweep_scores_side_workspace_bytes(const kge_murp_desc* d, int64_t n) {
    if (mu_check(d, "kge_murp_sweep_scores_side_workspace_bytes", false) || n < 0) return 0;
    return mu_eval_plan(d, n > 0 ? n : 1).total;
}

int kge_murp_eval_ranks(const kge_murp_desc* d, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                        const int64_t* head_off, const int32_t* head_ids, void* workspace, size_t workspace_bytes, int32_t* ranks,
                        int32_t* ties, void* stream) {
    const char* who = "kge_murp_eval_ranks";
    if (mu_check(d, who, false)) return -1;
    if (n < 0 || (n > 0 && (!triples || !ranks)) || (tail_off && !tail_ids) || (head_off && !head_ids)) {
        set_error("%s: bad arguments", who);
        return -1;
    }
    if (ws_check(who, workspace, workspace_bytes, mu_eval_plan(d, 2 * (n > 0 ? n : 1)).total)) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = debug_check_triples(who, d->tot_entity, d->tot_relation, triples, n, s)) return rc;
    const MuEval ev = mu_eval(d, workspace, 2 * n, 2);
    const MuArgs a = mu_args(d);
    if (hipMemsetAsync(ev.cnt, 0, (size_t)ev.nq * 2 * sizeof(int), s) != hipSuccess) { set_error("%s: hipMemsetAsync failed", who); return -2; }
    if (int rc = mu_queries(d, ev, triples, s)) return rc;
    hipLaunchKernelGGL(k_murp_truth, dim3((unsigned)((ev.nq + kMuBlock - 1) / kMuBlock)), dim3(kMuBlock), 0, s, a, ev, triples);
    if (int rc = check_launch("k_murp_truth")) return rc;
    if (int rc = mu_sweep(d, ev, nullptr, s)) return rc;
    hipLaunchKernelGGL(k_murp_finish, dim3((unsigned)((ev.nq + 3) / 4)), dim3(kMuBlock), 0, s, a, ev, triples, n, d->rank_order, tail_off,
                       tail_ids, head_off, head_ids, ranks, ties);
    return check_launch("k_murp_finish");
}

int kge_murp_sweep_scores_side(const kge_murp_desc* d, const int64_t* triples, int64_t n, int32_t side, void* workspace,
                               size_t workspace_bytes, double* scores, void* stream) {
    const char* who = "kge_murp_sweep_scores_side";
    if (mu_check(d, who, false)) return -1;
    if (n < 0 || (n > 0 && (!triples || !scores)) || (side != 0 && side != 1)) {
        set_error("%s: bad arguments (side is 0 = tail sweep or 1 = head sweep)", who);
        return -1;
    }
    if (ws_check(who, workspace, workspace_bytes, mu_eval_plan(d, n > 0 ? n : 1).total)) return -1;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = debug_check_triples(who, d->tot_entity, d->tot_relation, triples, n, s)) return rc;
    const MuEval ev = mu_eval(d, workspace, n, side);
    if (int rc = mu_queries(d, ev, triples, s)) return rc;
    return mu_sweep(d, ev, scores, s);
}

}  // extern "C"
