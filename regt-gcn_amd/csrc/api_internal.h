// What the host-only units of the C ABI (api_*.hip; map in DESIGN.md 6d) share.  No kernel unit includes this header.
#pragma once
#include <limits.h>

#include <functional>
#include <initializer_list>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "../../include/regtgcn.h"
#include "kernels.h"

#define TRY(x)               \
    do {                     \
        int _rc = (x);       \
        if (_rc) return _rc; \
    } while (0)

namespace regt {

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- api_runtime.hip ---------------------------------------------------------------------------------------------------------------
// optional per-kernel timing with HIP events (bench.py roofline)
// When enabled, every pipeline stage is bracketed by two events recorded on the launch stream.
struct ProfRec { const char* name; hipEvent_t e0, e1; };
extern bool g_prof_on;
extern std::vector<ProfRec> g_prof;
extern std::mutex g_prof_mu;

struct ProfScope {
    hipStream_t st; bool on; ProfRec r;
    ProfScope(const char* name, hipStream_t s) : st(s), on(g_prof_on) {
        if (!on) return;
        r.name = name;
        if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(r.e0, st);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(r.e1, st);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof.push_back(r);
    }
};
#define PROF(name, st) ProfScope _prof_scope_(name, st)

// per-call switches (regt_dims.flags) of the entry point running on this thread; the process-wide options are the defaults
extern thread_local unsigned t_call_flags;
// regt_dims.arith / .flags hold for the duration of one entry point on the calling thread
struct CallScope {
    int prev_mode;
    unsigned prev_flags;
    explicit CallScope(const regt_dims* d) {
        prev_flags = t_call_flags;
        t_call_flags = d ? d->flags : 0;
        const int a = d ? d->arith : 0;
        prev_mode = gemm_mode_override(a >= REGT_ARITH_FP32 && a <= REGT_ARITH_BF16 ? a - 1 : -1);
    }
    ~CallScope() { gemm_mode_override(prev_mode); t_call_flags = prev_flags; }
};

// hipGraph replay for launch-bound problem sizes (REGT_HIPGRAPH)
struct GraphEntry { hipGraphExec_t exec = nullptr; int seen = 0; };
struct GraphCache {
    std::unordered_map<unsigned long long, GraphEntry> map;
    std::mutex mu;
    long eager = 0, captured = 0, replayed = 0;
};
extern GraphCache g_fwd_graphs, g_bwd_graphs;
unsigned long long hash_bytes(const void* p, size_t n, unsigned long long h);
bool graphs_wanted(long rows);
// Runs `enqueue(stream)` either eagerly on `st` or as a cached graph replay ordered after / before `st`.
int run_maybe_graphed(GraphCache& cache, unsigned long long key, hipStream_t st, const std::function<int(hipStream_t)>& enqueue);

// library side stream of a launch stream, for work off the critical path
hipStream_t side_fork(hipStream_t st);      // returns the stream to launch on (st itself when the side stream is off)
int side_join(hipStream_t st);              // work forked to the side stream completes before what `st` gets next
void side_resync(hipStream_t st);

// ---- api_layout.hip ----------------------------------------------------------------------------------------------------------------
struct Layout {
    // saved by forward
    float *Xp, *AX, *LX, *h, *ZR, *q, *Ht, *y1, *probs;
    float *A0, *Aall, *bprime, *Gzr, *Gh, *czr, *ch;
    float *P0zr, *P1zr, *czr2;    // FMT_TCOLLAPSE: [Uz2; Ur2] W0, [Uz2; Ur2] W1 (2C x F each), czr + [Uz2; Ur2] b (2C)
    float *dP01;                  // ... and the gradient of [P0 | P1] (2C x 2F)
    float *S;    // (C, C): sum of the region blocks of tgnn.linear.weight (forward, reused by backward)
    // backward temporaries
    float *dOH, *d1, *dhp, *dzr, *dh, *dp_partial, *rowdot, *slab;
    float *UT;   // (3, C, C): transposed H-halves of the gate weights (h, z, r) for the data-gradient GEMMs
    float *Wb;   // fragment-order bf16 copies of the GEMM weights (bf16 mode)
    float *dA0, *dAall, *dbprime, *dGzr, *dGh, *dczr, *dch;
    int kchunk, nchunks, kchunk_s, nchunks_s, cb_npb, cb_blocks;
    long slab_floats;
    unsigned* tile_ctr;
    size_t bytes;
};
Layout make_layout(const regt_dims& d, int n_chunks_tab, int overlap, char* base);
Layout make_layout_fwd(const regt_dims& d, int overlap, bool fused, long x_rows, char* base);
Layout forward_only_layout(const regt_dims& d, const regt_graph& g, bool packed, int x_rows, bool xp_is_bf16, char* base, int* fmt);
// the zero-hidden cell
struct Layout0 {
    float *Z, *Ht, *y1, *probs, *dOH, *d1, *dzp, *dhp, *dp_partial, *slab;
    int kchunk, nchunks, cb_npb, cb_blocks;
    long slab_floats;
    size_t bytes;
};
Layout0 make_layout0(const regt_dims& d, int kz, int kh, char* base);
int check_dims(const regt_dims* d);

struct WbPtrs { const float *U[3], *UT[3], *Gzr, *Gh, *A0, *Aall; long ar_stride; };
WbPtrs wb_ptrs(const float* Wb, long C, long F);
struct HeadChunks { int k1, n1, k2, n2; };
HeadChunks head_chunks(long N, int H1, int C);

// ---- api_step.hip ------------------------------------------------------------------------------------------------------------------
// workspace formats remembered between forward and backward (note_q_format): bit 0 = bf16 intermediates, bit 1 = bf16 rows of
// x / A_hat x / L~ x, bit 2 = the packed input was the CALLER's bf16 buffer (else the rounded copy lives in the workspace)
// bit 4 = the forward ran with REGT_DIMS_FORWARD_ONLY: the workspace has the forward-only layout and holds nothing a backward could read
// bit 5 = the forward read the caller's packed rows (regt_forward_packed*): only the note of the workspace carries it, for regt_input_gradient
enum : int { FMT_QBF = 1, FMT_XBF = 2, FMT_XCALLER = 4, FMT_TCOLLAPSE = 8, FMT_FWDONLY = 16, FMT_PACKED = 32 };
bool bf16_intermediates(const regt_dims& d);
int forward_format(const regt_dims& d, const regt_graph& g, int x_rows, bool packed_fp32, bool xp_is_bf16);

inline GemmSeg make_seg(const float* A, long lda, const float* B0, const float* B1, long ldb, int nsplit, int K, bool bt,
                        int extra_flags = 0, long region_stride = 0) {
    GemmSeg s{};
    s.A = A; s.lda = lda; s.B0 = B0; s.B1 = B1 ? B1 : B0; s.ldb = ldb; s.nsplit = nsplit; s.K = K;
    s.b_region_stride = region_stride;
    int f = extra_flags | (bt ? SEG_BT : 0);
    if (lda % 4 == 0 && al16(A)) f |= SEG_VEC_A;
    if (ldb % 4 == 0 && al16(B0) && al16(s.B1) && region_stride % 4 == 0) f |= SEG_VEC_B;
    s.flags = f;
    return s;
}
// the GEMM of a single segment
inline GemmSegs one_seg(const GemmSeg& s, int row_div = 1) {
    GemmSegs S{};
    S.nseg = 1; S.seg[0] = s; S.row_div = row_div;
    return S;
}

// out[Nout x Nin] (+ column sums) = P^T Q over uniform chunks, reduced deterministically.
// Weight-gradient slabs and their reductions inside one backward pass: every wgrad gets its own slab region and its
// reduction is only recorded; flush() runs all recorded reductions in ONE launch.  A region request that does not fit
// flushes first and starts over at the base of the slab (stream order keeps that safe on `st`; the side stream is re-forked
// behind the flush, side_resync).
struct ReduceQueue {
    float* base;
    long capacity, used = 0;
    hipStream_t st;
    WgradReduceBatch batch{};
    ReduceQueue(float* b, long cap, hipStream_t s) : base(b), capacity(cap), st(s) {}
    int take(long floats, float** out) {
        floats = (floats + 63) & ~63L;
        REGT_CHECK_ARG(floats <= capacity, "backward: weight-gradient slab of %ld floats exceeds the workspace region (%ld)", floats, capacity);
        if (used + floats > capacity) {
            // the reduction just enqueued on `st` still reads the slabs: work on the side stream must not start overwriting
            // the region handed out next before it has run (side_join only orders `st` behind the side stream)
            TRY(flush());
            side_resync(st);
        }
        *out = base + used;
        used += floats;
        return REGT_OK;
    }
    int push(const WgradReduceArgs& r) {
        if (batch.n == WR_MAX_TASKS) TRY(flush_keep_slab());
        batch.t[batch.n++] = r;
        return REGT_OK;
    }
    int flush_keep_slab() {
        TRY(side_join(st));      // work forked to the library's side stream completes before any slab is reduced
        if (batch.n) {
            PROF("wgrad_reduce", st);
            TRY(launch_wgrad_reduce_multi(batch, st));
        }
        batch.n = 0;
        return REGT_OK;
    }
    int flush() {
        TRY(flush_keep_slab());
        used = 0;
        return REGT_OK;
    }
};
// The ONE weight-gradient path.  wgrad_launch takes the launch's slab region from the queue, launches under PROF(name) and gives back
// the region as a WgradSlab; every reduction of that slab is then `rq.push(w.block(...))`, which states only what differs: the block
// inside a slab, where it goes, and optionally its column sums or its chunk groups.
struct ReduceBlock : WgradReduceArgs {
    // column sums (bias gradient): `n` sums at slab element `offset` -> out (NULL: this block delivers none)
    ReduceBlock& colsum(float* out, long offset, int n) { colsum_out = out; colsum_offset = offset; ncolsum = n; return *this; }
    // chunk c belongs to output group chunk_group[c]; groups base .. base + n - 1 go to out + (group - base) * stride
    ReduceBlock& groups(const int* chunk_group_, int n, int base, long stride) {
        chunk_group = chunk_group_; ngroups = n; group_base = base; group_stride = stride;
        return *this;
    }
};
struct WgradSlab {
    float* slab; int nchunks; long stride; int row;      // `row`: output columns of the launch = length of a slab row
    // the (Nout x Nin) block at slab element `elem_offset` -> out with leading dimension ldo; a block narrower than the slab's rows
    // is strided by them (slab_ld), one that spans them is dense (slab_ld = 0)
    ReduceBlock block(long elem_offset, int Nout, int Nin, float* out, long ldo) const {
        ReduceBlock r{};
        r.slab = slab; r.nchunks = nchunks; r.slab_stride = stride; r.slab_ld = Nin == row ? 0 : row; r.ngroups = 1;
        r.elem_offset = elem_offset; r.Nout = Nout; r.Nin = Nin; r.out = out; r.ldo = ldo;
        return r;
    }
};
inline int wgrad_slab(ReduceQueue& q, int nchunks, long stride, int row, WgradSlab* w) {
    *w = WgradSlab{nullptr, nchunks, stride, row};
    return q.take((long)nchunks * stride, &w->slab);
}
inline int wgrad_launch(ReduceQueue& q, WgradArgs a, const char* name, hipStream_t st, WgradSlab* w) {
    TRY(wgrad_slab(q, a.nchunks, wgrad_slab_stride(a), a.Nin, w));
    a.slab = w->slab;
    PROF(name, st);
    return launch_wgrad(a, st);
}
// one gradient out[Nout x Nin] = P^T Q (+ column sums of P) over uniform chunks: launch and reduction
int wgrad_full(ReduceQueue& q, const char* name, const float* P, long ldp, int Nout, const float* Q, long ldq, int Nin, int q_relu,
               long M, int kchunk, int nchunks, float* out, long ldo, float* colsum, hipStream_t st, int p_bf16 = 0, int q_bf16 = 0);
int head_forward(const regt_dims& d, const regt_params& p, const float* hidden, float* y1, float* pred, hipStream_t st);
int head_backward(const regt_dims& d, const regt_params& p, const regt_grads& gr, const float* dpred, const float* dhidden,
                  const float* hidden, const float* y1, float* d1, float* dOH, ReduceQueue& rq, hipStream_t st);
int forward_impl(const regt_dims& d, const regt_graph& g, const regt_params& p, const float* x, const float* xp_ext, int x_rows,
                 float* pred, float* hidden, const Layout& L, hipStream_t st, bool skip_pack = false, const float* h_ext = nullptr, int fmt = 0);
int backward_impl(const regt_dims& d, const regt_graph& g, const regt_params& p, const regt_grads& gr, const float* dpred, const float* dhidden,
                  const float* hidden, const float* xp_ext, const Layout& L, hipStream_t st, int fmt, const float* h_ext = nullptr, float* dh_ext = nullptr);

}  // namespace regt
