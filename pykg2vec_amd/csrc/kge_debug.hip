// kge_debug.hip -- the id-range checks of the debug mode ("id-range checks (0 <= id < num_rows) in debug
// builds only").  The reference fails loudly on a bad id: nn.Embedding raises IndexError (models/Domain.py:8-13).  The
// kernels of this library index their tables with the ids they are handed and do not test them (a test per gathered row is
// not free, and batches produced by the device sampler are in range by construction), so an id beyond its table is an
// out-of-bounds read.  With KGE_DEBUG_IDS=1 in the environment (read once) or kge_set_debug(1), every entry point that takes
// ids from the caller first runs a scan kernel over them, waits for it, and returns -3 with the offending position in
// kge_last_error() instead of launching anything.  The scan synchronises the stream: the mode is for debugging, and it is
// skipped (with no effect on the call) while the stream is being captured into a hipGraph.
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include "kge_internal.h"

namespace kge {

struct SwitchOverride { char name[32]; int value; };
static SwitchOverride g_overrides[16];
static int g_n_overrides = 0;

int switch_value(const char* name) {
    for (int i = 0; i < g_n_overrides; ++i)
        if (!strcmp(g_overrides[i].name, name)) { if (g_overrides[i].value >= 0) return g_overrides[i].value; break; }
    char var[48];
    snprintf(var, sizeof(var), "KGE_%s", name);
    const char* e = getenv(var);
    if (!e || !e[0]) return -1;
    return atoi(e);
}
static int set_switch(const char* name, int value) {
    for (int i = 0; i < g_n_overrides; ++i)
        if (!strcmp(g_overrides[i].name, name)) { g_overrides[i].value = value; return 0; }
    if (g_n_overrides == 16 || strlen(name) >= sizeof(g_overrides[0].name)) return -1;
    strcpy(g_overrides[g_n_overrides].name, name);
    g_overrides[g_n_overrides++].value = value;
    return 0;
}

static int g_debug = -1;   // -1: environment not read yet

bool debug_ids() {
    if (g_debug < 0) {
        const char* e = getenv("KGE_DEBUG_IDS");
        g_debug = (e && e[0] && e[0] != '0') ? 1 : 0;
    }
    return g_debug > 0;
}
void set_debug_ids(int on) { g_debug = on ? 1 : 0; }

struct BadId { unsigned long long pos; long long value; };   // first = smallest position

// ids[i * stride + col] for i < n (perm != NULL: the rows perm[start + i] of an [*, stride] table); bound exclusive
__global__ __launch_bounds__(256) void k_check_ids(const int64_t* __restrict__ ids, const int64_t* __restrict__ perm, int64_t start,
                                                   int64_t n, int stride, int col, int64_t bound, unsigned long long* __restrict__ first,
                                                   long long* __restrict__ value) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = perm ? perm[start + i] : i;
        const int64_t v = ids[row * stride + col];
        if (v < 0 || v >= bound) {
            const unsigned long long old = atomicMin(first, (unsigned long long)i);
            if ((unsigned long long)i < old) *value = v;   // (racy among offenders, fine: any offender's value will do, the position is exact)
        }
    }
}
__global__ void k_check_ids32(const int32_t* __restrict__ ids, int64_t n, int stride, int col, int64_t bound,
                              unsigned long long* __restrict__ first, long long* __restrict__ value) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = ids[i * stride + col];
        if (v < 0 || v >= bound) {
            const unsigned long long old = atomicMin(first, (unsigned long long)i);
            if ((unsigned long long)i < old) *value = v;
        }
    }
}

// first position j inside a segment [off[i], off[i+1]) with ids[j] < ids[j-1] (the segments must be ascending; equal ids pass)
__global__ void k_check_ascending(const int64_t* __restrict__ off, const int32_t* __restrict__ ids, int64_t n,
                                  unsigned long long* __restrict__ first, long long* __restrict__ value) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        for (int64_t j = off[i] + 1; j < off[i + 1]; ++j) {
            if (ids[j] < ids[j - 1]) {
                const unsigned long long old = atomicMin(first, (unsigned long long)j);
                if ((unsigned long long)j < old) *value = ids[j];
                break;
            }
        }
    }
}

static BadId* g_flag = nullptr;   // 16 bytes of device memory, allocated on first use in debug mode only

static bool capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}

static int run_check(const char* who, const char* what, int64_t bound, hipStream_t s, void (*launch)(void*, BadId*, hipStream_t), void* ctx) {
    if (capturing(s)) return 0;
    if (!g_flag && hipMalloc(&g_flag, sizeof(BadId)) != hipSuccess) { set_error("%s: debug id check: hipMalloc failed", who); return -2; }
    BadId init{~0ull, 0};
    if (hipMemcpyAsync(g_flag, &init, sizeof(init), hipMemcpyHostToDevice, s) != hipSuccess) { set_error("%s: debug id check: copy failed", who); return -2; }
    launch(ctx, g_flag, s);
    BadId out;
    if (hipMemcpyAsync(&out, g_flag, sizeof(out), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: debug id check failed to run: %s", who, hipGetErrorString(hipGetLastError()));
        return -2;
    }
    if (out.pos != ~0ull && bound < 0) {
        set_error("%s: %s segments must be ascending: id %lld at position %llu is below its predecessor", who, what, out.value, out.pos);
        return -3;
    }
    if (out.pos != ~0ull) {
        set_error("%s: %s id out of range at position %llu: %lld not in [0, %lld) (an nn.Embedding lookup would raise IndexError, "
                  "models/Domain.py:8-13)", who, what, out.pos, out.value, (long long)bound);
        return -3;
    }
    return 0;
}

struct Ctx64 { const int64_t* ids; const int64_t* perm; int64_t start, n; int stride, col; int64_t bound; };
struct Ctx32 { const int32_t* ids; int64_t n; int stride, col; int64_t bound; };

static int grid_for(int64_t n) { int64_t b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }

int debug_check_ids(const char* who, const char* what, const int64_t* ids, int64_t n, int stride, int col, int64_t bound, hipStream_t s,
                    const int64_t* perm, int64_t start) {
    if (!debug_ids() || !ids || n <= 0) return 0;
    Ctx64 c{ids, perm, start, n, stride, col, bound};
    return run_check(who, what, bound, s, [](void* p, BadId* f, hipStream_t st) {
        const Ctx64& c = *(const Ctx64*)p;
        hipLaunchKernelGGL(k_check_ids, dim3(grid_for(c.n)), dim3(256), 0, st, c.ids, c.perm, c.start, c.n, c.stride, c.col, c.bound, &f->pos, &f->value);
    }, &c);
}

int debug_check_ids32(const char* who, const char* what, const int32_t* ids, int64_t n, int stride, int col, int64_t bound, hipStream_t s) {
    if (!debug_ids() || !ids || n <= 0) return 0;
    Ctx32 c{ids, n, stride, col, bound};
    return run_check(who, what, bound, s, [](void* p, BadId* f, hipStream_t st) {
        const Ctx32& c = *(const Ctx32*)p;
        hipLaunchKernelGGL(k_check_ids32, dim3(grid_for(c.n)), dim3(256), 0, st, c.ids, c.n, c.stride, c.col, c.bound, &f->pos, &f->value);
    }, &c);
}

struct CtxAsc { const int64_t* off; const int32_t* ids; int64_t n; };

int debug_check_ascending(const char* who, const char* what, const int64_t* off, const int32_t* ids, int64_t n, hipStream_t s) {
    if (!debug_ids() || !off || !ids || n <= 0) return 0;
    CtxAsc c{off, ids, n};
    return run_check(who, what, -1 /* no bound: the ascending-order message */, s, [](void* p, BadId* f, hipStream_t st) {
        const CtxAsc& c = *(const CtxAsc*)p;
        hipLaunchKernelGGL(k_check_ascending, dim3(grid_for(c.n)), dim3(256), 0, st, c.off, c.ids, c.n, &f->pos, &f->value);
    }, &c);
}

int debug_check_hrt(const char* who, const kge_model_desc* m, const int64_t* h, const int64_t* r, const int64_t* t, int64_t n, hipStream_t s) {
    if (!debug_ids()) return 0;
    int rc;
    if ((rc = debug_check_ids(who, "head", h, n, 1, 0, m->tot_entity, s))) return rc;
    if ((rc = debug_check_ids(who, "relation", r, n, 1, 0, m->tot_relation, s))) return rc;
    return debug_check_ids(who, "tail", t, n, 1, 0, m->tot_entity, s);
}

int debug_check_triples(const char* who, int64_t tot_entity, int64_t tot_relation, const int64_t* triples, int64_t n, hipStream_t s,
                        const int64_t* perm, int64_t start) {
    if (!debug_ids()) return 0;
    int rc;
    if ((rc = debug_check_ids(who, "head", triples, n, 3, 0, tot_entity, s, perm, start))) return rc;
    if ((rc = debug_check_ids(who, "relation", triples, n, 3, 1, tot_relation, s, perm, start))) return rc;
    return debug_check_ids(who, "tail", triples, n, 3, 2, tot_entity, s, perm, start);
}

__global__ void k_marker(int tag, int* sink) { if (sink && threadIdx.x == 0 && blockIdx.x == 0) *sink = tag; }

}  // namespace kge

extern "C" {
/* An empty launch of `tag` workgroups x 64 threads: a phase boundary a profiler trace can be cut at (bench.py's counter passes
 * cut the dispatch sequence of one process into per-configuration segments by the grid size of these launches). */
int kge_debug_marker(int32_t tag, void* stream) {
    if (tag < 1) { kge::set_error("kge_debug_marker: tag must be positive"); return -1; }
    hipLaunchKernelGGL(kge::k_marker, dim3((unsigned)tag), dim3(64), 0, (hipStream_t)stream, tag, (int*)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
int kge_set_switch(const char* name, int32_t value) {
    if (!name || kge::set_switch(name, value)) { kge::set_error("kge_set_switch: bad name or too many switches"); return -1; }
    return 0;
}
int kge_set_debug(int32_t check_ids) { kge::set_debug_ids(check_ids); return 0; }
int kge_get_debug(void) { return kge::debug_ids() ? 1 : 0; }
int kge_check_ids(const int64_t* ids, int64_t n, int64_t bound, void* stream) {
    // unconditional form of the scan (the host side uses it for id arrays it is about to hand to an index build)
    const bool was = kge::debug_ids();
    kge::set_debug_ids(1);
    const int rc = kge::debug_check_ids("kge_check_ids", "an", ids, n, 1, 0, bound, (hipStream_t)stream);
    kge::set_debug_ids(was);
    return rc;
}
}
