// kge_octonion.hip -- OctonionE (pointwise.py:772-1001): forward, backward, the fused pointwise-logistic step (explicit rows and
// sampler fused in front) and the rank sweep's candidate / query preparation.
//
// Tables come as two component blocks (include/kge_hip.h, KGE_OCTONIONE): entity component c (ent_embedding_{c+1}) starts at
// tables[0] + c * S_E floats, S_E = roundup4(E d), relation component c at tables[1] + c * S_R, S_R = roundup4(R d); grads[0] /
// grads[1] likewise.  With a = h_{1..4}, b = h_{5..8}, c = r^_{1..4}, d = r^_{5..8} (element-wise quaternions, r^ = r / |r|
// over the 8 components of each element) the reference composes
//     o = [a (x) c - d* (x) b | d (x) a + b (x) c*],   energy = -sum_k sum_c o_c t_c.
// The energy is bilinear in (h, r^) and linear in t.  With T1 = t_{1..4}, T2 = t_{5..8} the gradients of S = <o, t> are
//     dS/dt = o,  dS/da = T1 (x) c* + d* (x) T2,  dS/db = T2 (x) c - d (x) T1,
//     dS/dc = a* (x) T1 + T2* (x) b,  dS/dd = T2 (x) a* - b (x) T1*,
// and dS/dh = [dS/da | dS/db] is also the head query of the rank sweep.
//
// Every kernel walks its rows in chunks of G elements (lane gl holds element k0 + gl of all 8 components): 24 row values, the
// normalised relation and a few accumulators are live at a time, whatever d is -- no per-d register arrays, no scratch.
//
//   forward / backward   one lane group per triple; the backward scatters with float atomics
//   pointwise step       one lane group per bundle (a positive and its neg_rate corruptions, or `bundle` explicit rows): pass 1
//                        streams the chunks once per member for its energy (member k's lands in lane k), the logistic
//                        coefficients follow, pass 2 re-reads each chunk, forms the member gradients and the regulariser on the
//                        raw rows, sums the rows the member shares with the bundle's first row in registers and scatters them
//                        once per chunk
//   rank                 candidates [e_1 | ... | e_8] (K = 8d), query rows o(h, r^) (tail sweep) and dS/dh at t (head sweep), then
//                        the negated-dot pipeline of kge_eval.hip
#include "kge_row_kernels.h"

namespace kge {

constexpr int kOctMaxDim = 2048;

struct Quat { float s, x, y, z; };

__device__ __forceinline__ Quat qmul(Quat a, Quat b) {   // OctonionE._qmult, term order kept
    return Quat{a.s * b.s - a.x * b.x - a.y * b.y - a.z * b.z,
                a.s * b.x + b.s * a.x + a.y * b.z - b.y * a.z,
                a.s * b.y + b.s * a.y + a.z * b.x - b.z * a.x,
                a.s * b.z + b.s * a.z + a.x * b.y - b.x * a.y};
}
__device__ __forceinline__ Quat qconj(Quat a) { return Quat{a.s, -a.x, -a.y, -a.z}; }
__device__ __forceinline__ Quat qadd(Quat a, Quat b) { return Quat{a.s + b.s, a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ Quat qsub(Quat a, Quat b) { return Quat{a.s - b.s, a.x - b.x, a.y - b.y, a.z - b.z}; }

struct Oct { Quat lo, hi; };

__device__ __forceinline__ float oget(const Oct& o, int c) {
    const Quat& q = c < 4 ? o.lo : o.hi;
    const int j = c & 3;
    return j == 0 ? q.s : j == 1 ? q.x : j == 2 ? q.y : q.z;
}
__device__ __forceinline__ float& oref(Oct& o, int c) {
    Quat& q = c < 4 ? o.lo : o.hi;
    const int j = c & 3;
    return j == 0 ? q.s : j == 1 ? q.x : j == 2 ? q.y : q.z;
}
__device__ __forceinline__ Oct ozero() { return Oct{Quat{0.f, 0.f, 0.f, 0.f}, Quat{0.f, 0.f, 0.f, 0.f}}; }

// OctonionE._omult(h, r^)
__device__ __forceinline__ Oct omult(const Oct& h, const Oct& r) {
    return Oct{qsub(qmul(h.lo, r.lo), qmul(qconj(r.hi), h.hi)), qadd(qmul(r.hi, h.lo), qmul(h.hi, qconj(r.lo)))};
}
// dS/dh at (r^, t): the head query
__device__ __forceinline__ Oct grad_h(const Oct& r, const Oct& t) {
    return Oct{qadd(qmul(t.lo, qconj(r.lo)), qmul(qconj(r.hi), t.hi)), qsub(qmul(t.hi, r.lo), qmul(r.hi, t.lo))};
}
// dS/dr^ at (h, t)
__device__ __forceinline__ Oct grad_r(const Oct& h, const Oct& t) {
    return Oct{qadd(qmul(qconj(h.lo), t.lo), qmul(qconj(t.hi), h.hi)), qsub(qmul(t.hi, qconj(h.lo)), qmul(h.hi, qconj(t.lo)))};
}

struct OctArgs {
    const float* ent; const float* rel;   // component blocks
    float* gent; float* grel;
    int64_t se, sr;                       // component strides (floats)
    int d;
};

// element k of the 8 components of row `row` (k < d, else zeros).  The component base is uniform and the lane's offset a 32-bit
// element index (a component holds fewer than 2^32 floats), so each access is one scalar base plus one VGPR instead of 8 64-bit
// lane addresses per row.
__device__ __forceinline__ Oct load_oct(const float* __restrict__ base, int64_t stride, int64_t row, int d, int k) {
    Oct o = ozero();
    if (k < d) {
        const uint32_t off = (uint32_t)(row * d + k);
#pragma unroll
        for (int c = 0; c < 8; ++c) oref(o, c) = (base + c * stride)[off];
    }
    return o;
}
__device__ __forceinline__ void atomic_oct(float* __restrict__ base, int64_t stride, int64_t row, int d, int k, const Oct& g) {
    if (k >= d) return;
    const uint32_t off = (uint32_t)(row * d + k);
#pragma unroll
    for (int c = 0; c < 8; ++c) unsafeAtomicAdd((base + c * stride) + off, oget(g, c));
}

// OctonionE._onorm per element: r / sqrt(sum_c r_c^2), no eps; a zero norm gives zeros (as QuatE's kernel does)
__device__ __forceinline__ Oct onorm(const Oct& r, float& den) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) s += oget(r, c) * oget(r, c);
    den = sqrtf(s);
    Oct o;
#pragma unroll
    for (int c = 0; c < 8; ++c) oref(o, c) = den > 0.f ? oget(r, c) / den : 0.f;
    return o;
}
// d/dr of g . r^: (g - r^ (r^ . g)) / |r|
__device__ __forceinline__ Oct onorm_bwd(const Oct& g, const Oct& rn, float den) {
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) dot = fmaf(oget(rn, c), oget(g, c), dot);
    Oct o;
#pragma unroll
    for (int c = 0; c < 8; ++c) oref(o, c) = den > 0.f ? (oget(g, c) - oget(rn, c) * dot) / den : 0.f;
    return o;
}

__device__ __forceinline__ float odot(const Oct& a, const Oct& b) {   // o_1 t_1 + ... + o_8 t_8, the reference's order
    float s = oget(a, 0) * oget(b, 0);
#pragma unroll
    for (int c = 1; c < 8; ++c) s += oget(a, c) * oget(b, c);
    return s;
}
__device__ __forceinline__ void oaxpy(Oct& y, float a, const Oct& x) {
#pragma unroll
    for (int c = 0; c < 8; ++c) oref(y, c) = fmaf(a, oget(x, c), oget(y, c));
}

// ---------------------------------------------------------------- forward / backward: one lane group per triple
template <int G, bool BWD>
__global__ __launch_bounds__(kBlock) void k_oct_score(OctArgs a, const int64_t* __restrict__ h, const int64_t* __restrict__ r,
                                                      const int64_t* __restrict__ t, int64_t n, float* __restrict__ scores,
                                                      const float* __restrict__ dscore) {
    constexpr int GPB = kBlock / G;
    const int gl = threadIdx.x % G;
    for (int64_t i = (int64_t)blockIdx.x * GPB + threadIdx.x / G; i < n; i += (int64_t)gridDim.x * GPB) {
        float ds = 0.f;
        if constexpr (BWD) {
            ds = dscore[i];
            if (ds == 0.f) continue;   // group-uniform
        }
        const int64_t hi = h[i], ri = r[i], ti = t[i];
        float p = 0.f;
        for (int k0 = 0; k0 < a.d; k0 += G) {
            const int k = k0 + gl;
            const Oct hv = load_oct(a.ent, a.se, hi, a.d, k), tv = load_oct(a.ent, a.se, ti, a.d, k);
            float den;
            const Oct rn = onorm(load_oct(a.rel, a.sr, ri, a.d, k), den);
            if constexpr (!BWD) {
                p += odot(omult(hv, rn), tv);
            } else {
                // energy = -S: d(ds * energy) = -ds dS
                Oct gh = ozero(), gt = ozero(), gr = ozero();
                oaxpy(gh, -ds, grad_h(rn, tv));
                oaxpy(gt, -ds, omult(hv, rn));
                oaxpy(gr, -ds, grad_r(hv, tv));
                atomic_oct(a.gent, a.se, hi, a.d, k, gh);
                atomic_oct(a.gent, a.se, ti, a.d, k, gt);
                atomic_oct(a.grel, a.sr, ri, a.d, k, onorm_bwd(gr, rn, den));
            }
        }
        if constexpr (!BWD) {
            const float s = gsum<G>(p);
            if (gl == 0) scores[i] = -s;
        }
    }
}

// regulariser of one raw row element: loss part and gradient (coefficients c2 = 2 lmbda / n, c3 = 3 lmbda / n)
__device__ __forceinline__ void oct_reg(const Oct& x, int reg_type, float c2, float c3, float& part, Oct& g) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float v = oget(x, c);
        if (reg_type == KGE_REG_F2) { part = fmaf(v, v, part); oref(g, c) += c2 * v; }
        else if (reg_type == KGE_REG_N3) { part += v * v * v; oref(g, c) += c3 * v * v; }
        else { const float av = fabsf(v); part += av * av * av; oref(g, c) += c3 * v * av; }
    }
}

// ---------------------------------------------------------------- fused pointwise-logistic step: one lane group per bundle
template <int G>
__global__ __launch_bounds__(kBlock) void k_oct_pointwise(OctArgs a, const int64_t* __restrict__ h, const int64_t* __restrict__ r,
                                                          const int64_t* __restrict__ t, const int64_t* __restrict__ y, int64_t n,
                                                          int bundle, float lmbda, int reg_type, float* __restrict__ loss,
                                                          FusedSampler fs) {
    constexpr int GPB = kBlock / G;
    const int gl = threadIdx.x % G;
    const int gbase = (threadIdx.x & 63) / G * G;
    const bool sampled = fs.triples != nullptr;
    const int64_t s_start = (sampled && fs.cursor) ? fs.start + fs.cursor[0] : fs.start;
    const unsigned long long s_off = (sampled && fs.cursor) ? fs.offset + (unsigned long long)fs.cursor[1] : fs.offset;
    const float inv_n = 1.0f / (float)n;
    const float c2 = 2.f * lmbda * inv_n, c3 = 3.f * lmbda * inv_n;
    const bool reg = reg_type == KGE_REG_F2 || reg_type == KGE_REG_N3 || reg_type == KGE_REG_N3_ABS;
    const int64_t nb = (n + bundle - 1) / bundle;
    float acc = 0.f;     // this lane's share of the loss: its member's softplus term, its elements' regulariser terms
    for (int64_t b = (int64_t)blockIdx.x * GPB + threadIdx.x / G; b < nb; b += (int64_t)gridDim.x * GPB) {
        const int64_t i0 = b * bundle;
        const int nm = (int)(min(n, i0 + bundle) - i0);
        int64_t pos[3];
        int my_nh = 0, my_nt = 0;
        if (sampled) {
            const int64_t row = fs.perm[s_start + b];
            pos[0] = fs.triples[3 * row]; pos[1] = fs.triples[3 * row + 1]; pos[2] = fs.triples[3 * row + 2];
            if (gl < bundle - 1) {
                int64_t nh, nt;
                corrupt_one(pos[0], pos[1], pos[2], fs.E, fs.bern, fs.slots, fs.mask, fs.seed,
                            s_off + (unsigned long long)(b * (bundle - 1) + gl), nh, nt);
                my_nh = (int)nh; my_nt = (int)nt;
            }
        } else {
            pos[0] = h[i0]; pos[1] = r[i0]; pos[2] = t[i0];
        }
        // member k of the bundle (group-uniform k)
        auto member = [&](int k, int64_t& mh, int64_t& mr, int64_t& mt, float& my) {
            if (sampled) {
                const int src = gbase + (k > 0 ? k - 1 : 0);
                const int nh = __shfl(my_nh, src, 64), nt = __shfl(my_nt, src, 64);
                mh = k == 0 ? pos[0] : (int64_t)nh; mr = pos[1]; mt = k == 0 ? pos[2] : (int64_t)nt;
                my = k == 0 ? 1.f : -1.f;
            } else {
                mh = h[i0 + k]; mr = r[i0 + k]; mt = t[i0 + k];
                my = (float)y[i0 + k];
            }
        };
        // pass 1: member k's energy in lane k, its loss term and coefficient d(loss)/d(energy)
        float my_ds = 0.f;
        for (int k = 0; k < nm; ++k) {
            int64_t mh, mr, mt;
            float my;
            member(k, mh, mr, mt, my);
            float p = 0.f;
            for (int k0 = 0; k0 < a.d; k0 += G) {
                const int e = k0 + gl;
                float den;
                const Oct rn = onorm(load_oct(a.rel, a.sr, mr, a.d, e), den);
                p += odot(omult(load_oct(a.ent, a.se, mh, a.d, e), rn), load_oct(a.ent, a.se, mt, a.d, e));
            }
            const float x = my * -gsum<G>(p);
            if (gl == k) {
                acc += softplus_t(x) * inv_n;
                my_ds = my * sigmoid_t(x) * inv_n;
            }
            if (reg_type >= KGE_REG_ID_F2 && gl == 0) {
                const int64_t id[3] = {mh, mr, mt};
                acc += id_reg_term(id, lmbda, reg_type);
            }
        }
        // pass 2: chunk by chunk, rows shared with the first member accumulate in registers and scatter once
        for (int k0 = 0; k0 < a.d; k0 += G) {
            const int e = k0 + gl;
            const Oct ra = load_oct(a.rel, a.sr, pos[1], a.d, e);
            float dena;
            const Oct rna = onorm(ra, dena);
            Oct Ah = ozero(), At = ozero(), Ar = ozero();   // Ar: d/dr^ of the anchor relation (normalisation backward at the flush)
            int nra = 0;                                    // members on the anchor relation (the raw-row regulariser counts each)
            for (int k = 0; k < nm; ++k) {
                int64_t mh, mr, mt;
                float my;
                member(k, mh, mr, mt, my);
                const float g = -__shfl(my_ds, gbase + k, 64);   // d(loss)/dS = -d(loss)/d(energy)
                const Oct hv = load_oct(a.ent, a.se, mh, a.d, e), tv = load_oct(a.ent, a.se, mt, a.d, e);
                const bool own_rel = mr == pos[1];              // group-uniform
                Oct rv = ra, rn = rna;
                float den = dena;
                if (!own_rel) {
                    rv = load_oct(a.rel, a.sr, mr, a.d, e);
                    rn = onorm(rv, den);
                }
                Oct gh = ozero(), gt = ozero(), gr = ozero();
                oaxpy(gh, g, grad_h(rn, tv));
                oaxpy(gt, g, omult(hv, rn));
                oaxpy(gr, g, grad_r(hv, tv));
                if (reg) {
                    float part = 0.f;
                    oct_reg(hv, reg_type, c2, c3, part, gh);
                    oct_reg(tv, reg_type, c2, c3, part, gt);
                    Oct greg = ozero();
                    oct_reg(rv, reg_type, c2, c3, part, greg);
                    acc += lmbda * inv_n * part;
                    if (!own_rel) {
                        Oct gfull = onorm_bwd(gr, rn, den);
#pragma unroll
                        for (int c = 0; c < 8; ++c) oref(gfull, c) += oget(greg, c);
                        atomic_oct(a.grel, a.sr, mr, a.d, e, gfull);
                    }
                } else if (!own_rel) {
                    atomic_oct(a.grel, a.sr, mr, a.d, e, onorm_bwd(gr, rn, den));
                }
                if (own_rel) {
                    ++nra;
#pragma unroll
                    for (int c = 0; c < 8; ++c) oref(Ar, c) += oget(gr, c);
                }
                if (mh == pos[0]) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) oref(Ah, c) += oget(gh, c);
                } else {
                    atomic_oct(a.gent, a.se, mh, a.d, e, gh);
                }
                if (mt == pos[2]) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) oref(At, c) += oget(gt, c);
                } else {
                    atomic_oct(a.gent, a.se, mt, a.d, e, gt);
                }
            }
            Oct gra = onorm_bwd(Ar, rna, dena);
            if (reg) {
                Oct greg = ozero();
                float unused = 0.f;
                oct_reg(ra, reg_type, c2, c3, unused, greg);
                oaxpy(gra, (float)nra, greg);
            }
            atomic_oct(a.grel, a.sr, pos[1], a.d, e, gra);
            atomic_oct(a.gent, a.se, pos[0], a.d, e, Ah);
            atomic_oct(a.gent, a.se, pos[2], a.d, e, At);
        }
    }
    block_accumulate_loss<G>(gsum<G>(acc), gl, loss);
}

// ---------------------------------------------------------------- host side
static int64_t roundup4(int64_t x) { return (x + 3) & ~(int64_t)3; }
static int oct_group(int d) { return d <= 256 ? 32 : 64; }   // the lane group: also the most negatives a sampled bundle may draw

static int oct_check(const kge_model_desc* m, const char* who) {
    if (m->model != KGE_OCTONIONE) { set_error("%s: not an OctonionE descriptor (model %d)", who, m->model); return -1; }
    if (m->dim > kOctMaxDim) { set_error("%s: OctonionE takes hidden sizes 1..%d (got %d)", who, kOctMaxDim, m->dim); return -1; }
    if (m->tot_entity * (int64_t)m->dim >= (int64_t(1) << 32) || m->tot_relation * (int64_t)m->dim >= (int64_t(1) << 32)) {
        set_error("%s: a component of more than 2^32 floats (the kernels index a component with 32-bit offsets)", who);
        return -1;
    }
    return 0;
}

static OctArgs oct_args(const kge_model_desc* m) {
    return OctArgs{m->tables[0], m->tables[1], m->grads[0], m->grads[1], roundup4(m->tot_entity * (int64_t)m->dim),
                   roundup4(m->tot_relation * (int64_t)m->dim), m->dim};
}

static unsigned oct_blocks(int64_t items, int G) {
    const int64_t gpb = kBlock / G;
    int64_t b = (items + gpb - 1) / gpb;
    if (b > kMaxBlocks) b = kMaxBlocks;
    return (unsigned)(b < 1 ? 1 : b);
}

static int oct_score(const kge_model_desc* m, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n, float* scores,
                     const float* dscore, hipStream_t s) {
    if (oct_check(m, dscore ? "kge_score_backward" : "kge_score_forward")) return -1;
    if (n <= 0) return 0;
    const OctArgs a = oct_args(m);
    const int G = oct_group(m->dim);
    const dim3 grid(oct_blocks(n, G)), block(kBlock);
    if (dscore) {
        if (G == 32) hipLaunchKernelGGL((k_oct_score<32, true>), grid, block, 0, s, a, h, r, t, n, nullptr, dscore);
        else hipLaunchKernelGGL((k_oct_score<64, true>), grid, block, 0, s, a, h, r, t, n, nullptr, dscore);
        return check_launch("k_oct_score<backward>");
    }
    if (G == 32) hipLaunchKernelGGL((k_oct_score<32, false>), grid, block, 0, s, a, h, r, t, n, scores, nullptr);
    else hipLaunchKernelGGL((k_oct_score<64, false>), grid, block, 0, s, a, h, r, t, n, scores, nullptr);
    return check_launch("k_oct_score<forward>");
}

// (table signatures: no scorer workspace, the one handed in is ignored)
int launch_octonion_forward(const kge_model_desc* m, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n, float* scores,
                            void*, size_t, hipStream_t s) {
    return oct_score(m, h, r, t, n, scores, nullptr, s);
}

int launch_octonion_backward(const kge_model_desc* m, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n,
                             const float* dscore, void*, size_t, hipStream_t s) {
    return oct_score(m, h, r, t, n, nullptr, dscore, s);
}

static int oct_pointwise(const kge_model_desc* m, const int64_t* h, const int64_t* r, const int64_t* t, const int64_t* y, int64_t n,
                         int bundle, float lmbda, int reg_type, float* loss, const FusedSampler& fs, hipStream_t s) {
    const OctArgs a = oct_args(m);
    const int G = oct_group(m->dim);
    const dim3 grid(oct_blocks((n + bundle - 1) / bundle, G)), block(kBlock);
    if (G == 32) hipLaunchKernelGGL((k_oct_pointwise<32>), grid, block, 0, s, a, h, r, t, y, n, bundle, lmbda, reg_type, loss, fs);
    else hipLaunchKernelGGL((k_oct_pointwise<64>), grid, block, 0, s, a, h, r, t, y, n, bundle, lmbda, reg_type, loss, fs);
    return check_launch("k_oct_pointwise");
}

int launch_octonion_pointwise(const kge_model_desc* m, const int64_t* h, const int64_t* r, const int64_t* t, const int64_t* y,
                              int64_t n, int bundle, float lmbda, int reg_type, float* loss, hipStream_t s) {
    if (oct_check(m, "kge_train_pointwise_logistic")) return -1;
    if (n <= 0) return 0;
    // a member's energy waits in lane k of the group between the passes: longer bundles run row by row (exact either way)
    if (bundle < 1 || bundle > oct_group(m->dim)) bundle = 1;
    return oct_pointwise(m, h, r, t, y, n, bundle, lmbda, reg_type, loss, FusedSampler{}, s);
}

int launch_octonion_pointwise_sampled(const kge_model_desc* m, const int64_t* triples, const int64_t* perm, int64_t start,
                                      int64_t n_pos, int neg_rate, const float* bern, const uint64_t* slots, int64_t n_slots,
                                      uint64_t seed, uint64_t offset, const int64_t* cursor, float lmbda, int reg_type, float* loss,
                                      hipStream_t s) {
    const char* who = "kge_train_pointwise_logistic_sampled";
    if (oct_check(m, who)) return -1;
    if (n_pos <= 0) return 0;
    // the bundle's positive sits in lane 0 and negative j's draw in lane j, so 1 + neg_rate rows must fit one lane group
    if (1 + neg_rate > oct_group(m->dim)) {
        set_error("%s: OctonionE with hidden size %d takes neg_rate <= %d", who, m->dim, oct_group(m->dim) - 1);
        return -1;
    }
    FusedSampler fs;
    fs.triples = triples; fs.perm = perm; fs.start = start; fs.E = m->tot_entity; fs.bern = bern;
    fs.slots = (const unsigned long long*)slots; fs.mask = (unsigned long long)(slots ? n_slots - 1 : 0);
    fs.seed = seed; fs.offset = offset; fs.cursor = cursor;
    return oct_pointwise(m, nullptr, nullptr, nullptr, nullptr, n_pos * (1 + (int64_t)neg_rate), 1 + neg_rate, lmbda, reg_type, loss,
                         fs, s);
}

// ---------------------------------------------------------------- rank: candidates, query rows, the negated-dot pipeline
// one thread per (entity, element): cand[e][c d + k] = ent_{c+1}[e][k]
__global__ __launch_bounds__(kBlock) void k_oct_cand(const float* __restrict__ ent, int64_t se, int64_t E, int d,
                                                     float* __restrict__ cand) {
    const int64_t total = E * d;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t e = i / d;
        const int k = (int)(i - e * d);
        float* o = cand + e * (int64_t)(8 * d) + k;
#pragma unroll
        for (int c = 0; c < 8; ++c) o[c * d] = ent[c * se + i];
    }
}

// one thread per (test triple, element): row 2i = o(h, r^) (tail sweep), row 2i + 1 = dS/dh at (r^, t) (head sweep), width 8d
__global__ __launch_bounds__(kBlock) void k_oct_queries(OctArgs a, const int64_t* __restrict__ triples, int64_t n,
                                                        float* __restrict__ qrows) {
    const int d = a.d;
    const int64_t total = n * d;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < total; j += (int64_t)gridDim.x * kBlock) {
        const int64_t i = j / d;
        const int k = (int)(j - i * d);
        const int64_t hi = triples[3 * i], ri = triples[3 * i + 1], ti = triples[3 * i + 2];
        float den;
        const Oct rn = onorm(load_oct(a.rel, a.sr, ri, d, k), den);
        const Oct qt = omult(load_oct(a.ent, a.se, hi, d, k), rn);
        const Oct qh = grad_h(rn, load_oct(a.ent, a.se, ti, d, k));
        float* ot = qrows + 2 * i * (int64_t)(8 * d) + k;
        float* oh = ot + 8 * d;
#pragma unroll
        for (int c = 0; c < 8; ++c) { ot[c * d] = oget(qt, c); oh[c * d] = oget(qh, c); }
    }
}

size_t octonion_eval_workspace_bytes(const kge_model_desc* m, int64_t n) {
    if (m->dim > kOctMaxDim) return 0;
    const DotRowsPlan w = dot_rows_plan(nullptr, m->tot_entity, n, 8 * m->dim);
    return w.pipe_bytes ? w.bytes : 0;
}

int launch_octonion_eval(const kge_model_desc* m, const int64_t* triples, int64_t n, const int64_t* tail_off, const int32_t* tail_ids,
                         const int64_t* head_off, const int32_t* head_ids, void* ws, size_t ws_bytes, int32_t* ranks, int32_t* ties,
                         float* scores, hipStream_t s, int side) {
    if (oct_check(m, "kge_eval")) return -1;
    const DotRowsPlan w = dot_rows_plan(ws, m->tot_entity, n, 8 * m->dim);
    if (!ws || ws_bytes < w.bytes) { set_error("kge_eval (OctonionE): workspace too small (%zu < %zu)", ws_bytes, w.bytes); return -1; }
    if (n <= 0) return 0;
    const OctArgs a = oct_args(m);
    const int64_t E = m->tot_entity;
    const int d = m->dim;
    auto blocks = [](int64_t items) {
        int64_t b = (items + kBlock - 1) / kBlock;
        return (unsigned)(b > 4 * kMaxBlocks ? 4 * kMaxBlocks : (b < 1 ? 1 : b));
    };
    hipLaunchKernelGGL(k_oct_cand, dim3(blocks(E * d)), dim3(kBlock), 0, s, a.ent, a.se, E, d, w.cand);
    hipLaunchKernelGGL(k_oct_queries, dim3(blocks(n * d)), dim3(kBlock), 0, s, a, triples, n, w.qrows);
    if (int rc = check_launch("k_oct_cand / k_oct_queries")) return rc;
    return launch_dot_eval(w.cand, w.qrows, 8 * d, E, triples, n, tail_off, tail_ids, head_off, head_ids, w.pipe, w.pipe_bytes,
                           ranks, ties, scores, s, side);
}

}  // namespace kge
