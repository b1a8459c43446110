// Launch-plan recorder of the training step (tests/test_step_plan_cpu.py).  Links csrc/api_step.hip and csrc/api_layout.hip compiled
// host-only and stands in for everything else they call: every launch_* appends one line to a log -- its name and every field the
// kernel would read, field by field -- instead of launching.  Pointers are fake, never dereferenced, and printed as arena+offset.
//   step_plan            per case and launch: name and a 64-bit FNV-1a hash of the canonical field text (tests/golden/step_plan.txt)
//   step_plan --full     the canonical text itself
// The predicates and chunk rules below are simple deterministic stand-ins: the recorder pins the step's logic GIVEN their answers.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#include "api_internal.h"

namespace {

// ---- the case at hand ------------------------------------------------------------------------------------------------------------
struct Case {
    const char* name = "";
    int N = 40, T = 12, F = 32, C = 256, R = 5, O = 1, H1 = 128, regional = 1;
    int mode = 0;                   // gemm_mode(): 0 fp32, 1 bf16x3, 2 bf16
    unsigned flags = 0;             // regt_dims.flags of the call
    int overlap = 0, region_lo = 0, region_hi = 0, sorted = 1;
    bool attention = true;          // gr.attention != NULL
    bool wide = false;              // fp32_core_wide()
    bool embed_ok = true, gen_ok = true;
    bool cell = false;              // regt_cell_forward / _backward: h_ext, dh_ext
    bool fwd_only = false;          // REGT_DIMS_FORWARD_ONLY: no backward
    bool caller_bf16 = false;       // regt_forward_packed_bf16
    bool min_slab = false;          // slab region = the largest single request
    int opt[regt::OPT_COUNT];
    Case() {
        for (int& o : opt) o = 0;
        opt[regt::OPT_XBF] = opt[regt::OPT_FUSED_BWD] = opt[regt::OPT_TGCN_COLLAPSE] = opt[regt::OPT_DGRAD1_GEN] = 1;
        opt[regt::OPT_FUSED_ROWS] = opt[regt::OPT_EMBED_KERNEL] = opt[regt::OPT_WGRAD_BNW64] = opt[regt::OPT_WGRAD_WAVE] = 1;
        opt[regt::OPT_WGRAD_RING] = 6; opt[regt::OPT_WGRAD_TILE] = 256; opt[regt::OPT_WGRAD_RING256] = 2; opt[regt::OPT_WGRAD_PAIRS] = 2;
        opt[regt::OPT_SIDE_STREAM] = 1;
    }
};
Case g_case;

// ---- fake arenas -----------------------------------------------------------------------------------------------------------------
constexpr unsigned long long ARENA0 = 0x100000000000ull, ARENA_STEP = 0x4000000000ull;      // 256 GB apart, 16-byte aligned
std::vector<std::string> g_arenas;
float* arena(const char* name) {
    g_arenas.push_back(name);
    return reinterpret_cast<float*>(ARENA0 + (g_arenas.size() - 1) * ARENA_STEP);
}
std::string ptr_name(const void* p) {
    if (!p) return "null";
    const unsigned long long a = reinterpret_cast<unsigned long long>(p);
    char buf[96];
    if (a >= ARENA0 && (a - ARENA0) / ARENA_STEP < g_arenas.size()) {
        snprintf(buf, sizeof buf, "%s+%llu", g_arenas[(a - ARENA0) / ARENA_STEP].c_str(), (a - ARENA0) % ARENA_STEP);
    } else {
        snprintf(buf, sizeof buf, "stray:%llx", a);
    }
    return buf;
}
const hipStream_t MAIN = reinterpret_cast<hipStream_t>(0x1000), SIDE = reinterpret_cast<hipStream_t>(0x2000);
const char* stream_name(hipStream_t s) { return s == MAIN ? "main" : s == SIDE ? "side" : "stream?"; }

// ---- the log ---------------------------------------------------------------------------------------------------------------------
struct Rec { std::string name, text; std::vector<int> scopes; };
std::vector<Rec> g_log;
std::vector<int> g_open;                     // PROF scopes open now: ids of their first event
std::vector<hipStream_t> g_event_stream;     // per event id
long g_max_take = 0;                         // largest slab request seen (64-float granules, as ReduceQueue::take rounds)

struct Line {
    Rec r;
    explicit Line(const char* name) { r.name = name; r.scopes = g_open; }
    ~Line() { g_log.push_back(r); }
    void add(const char* k, const std::string& v) { r.text += ' '; r.text += k; r.text += '='; r.text += v; }
    Line& p(const char* k, const void* v) { add(k, ptr_name(v)); return *this; }
    Line& i(const char* k, long long v) { add(k, std::to_string(v)); return *this; }
    Line& f(const char* k, float v) { char b[40]; snprintf(b, sizeof b, "%.9g", v); add(k, b); return *this; }
    Line& s(hipStream_t st) { add("stream", stream_name(st)); return *this; }
    Line& segs(const regt::GemmSegs& S) {
        i("nseg", S.nseg).p("node_region", S.node_region).i("row_div", S.row_div).i("num_regions", S.num_regions);
        for (int k = 0; k < S.nseg; ++k) {
            const regt::GemmSeg& g = S.seg[k];
            i("seg", k).p("A", g.A).i("lda", g.lda).p("B0", g.B0).p("B1", g.B1).i("ldb", g.ldb).i("nsplit", g.nsplit).i("K", g.K)
                .i("flags", g.flags).i("b_region_stride", g.b_region_stride).i("a_rep_stride", g.a_rep_stride).i("nrep", g.nrep);
        }
        return *this;
    }
};

unsigned long long fnv1a(const std::string& s) {
    unsigned long long h = 0xcbf29ce484222325ull;
    for (unsigned char c : s) { h ^= c; h *= 0x100000001b3ull; }
    return h;
}

}  // namespace

// ---- HIP events of ProfScope: profiling is ON in the recorder so that every PROF scope leaves its name (g_prof) --------------------
extern "C" hipError_t hipEventCreate(hipEvent_t* e) {
    g_event_stream.push_back(nullptr);
    *e = reinterpret_cast<hipEvent_t>(g_event_stream.size());      // id + 1: never NULL
    return hipSuccess;
}
extern "C" hipError_t hipEventRecord(hipEvent_t e, hipStream_t st) {
    const int id = (int)reinterpret_cast<unsigned long long>(e) - 1;
    g_event_stream[id] = st;
    if (id % 2 == 0) g_open.push_back(id);      // ProfScope creates e0, e1 in this order: even ids open a scope, odd ids close it
    else g_open.pop_back();
    return hipSuccess;
}

namespace regt {

bool g_prof_on = true;
std::vector<ProfRec> g_prof;
std::mutex g_prof_mu;
thread_local unsigned t_call_flags = 0;

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    Line("set_error").add("text", buf);
}

// ---- switches and predicates: from the case ------------------------------------------------------------------------------------------
int option(OptId id) { return g_case.opt[id]; }
int gemm_mode() { return g_case.mode; }
int gemm_mode_override(int) { return -1; }
bool fp32_core_wide() { return g_case.wide; }
bool gemm_desc_table_forced() { return false; }
bool fused_forward_ok(int C, int F) { return C == 256 && F == 64; }
bool fused_forward_rows_ok(int C, int F, int T) { return C == 256 && (F == 32 || F == 64) && T <= 16; }
bool fused_backward_ok(int C) { return C == 256; }
bool head2_skinny_ok(int H1, int O, const void* y1, const void* W2) { return O <= 4 && H1 % 4 == 0 && al16(y1) && al16(W2); }
bool embed_fp32_ok(long, int C, int F, int) { return g_case.embed_ok && C == 256 && F == 32; }
bool gemm_dgrad1_gen_ok(long, int C, int) { return g_case.gen_ok && option(OPT_DGRAD1_GEN) && gemm_mode() < 2 && !fp32_core_wide() && C % 128 == 0; }
bool wgrad_ring_active() { return option(OPT_WGRAD_RING) > 0; }
// three different chunk lengths, so that the log shows which rule a launch took
static bool chunks_of(long rows, long M, int* kchunk, int* nchunks) { *kchunk = (int)rows; *nchunks = (int)((M + rows - 1) / rows); return true; }
bool wgrad_ring_chunking(int, int, long M, int* kchunk, int* nchunks) { return chunks_of(96, M, kchunk, nchunks); }
bool wgrad_skinny_chunking(int, long M, int* kchunk, int* nchunks) { return chunks_of(64, M, kchunk, nchunks); }
bool wgrad_wide_chunking(int, int, long M, int* kchunk, int* nchunks) { return chunks_of(160, M, kchunk, nchunks); }
long wgrad_chunk_bound(int, int, long M) { return (M + 63) / 64; }
long wgrad_slab_stride(const WgradArgs& a) { return (long)a.Nout * a.Nin + (a.colsum ? a.Nout : 0); }
int cell_bwd_blocks(int num_nodes, int nodes_per_block) { return (num_nodes + nodes_per_block - 1) / nodes_per_block; }

// ---- side stream -------------------------------------------------------------------------------------------------------------------------
static bool side_on() { return option(OPT_SIDE_STREAM) && !(t_call_flags & REGT_DIMS_NO_SIDE_STREAM); }
hipStream_t side_fork(hipStream_t st) { Line("side_fork").s(st); return side_on() ? SIDE : st; }
int side_join(hipStream_t st) { Line("side_join").s(st); return REGT_OK; }
void side_resync(hipStream_t st) { Line("side_resync").s(st); }

// ---- launchers -----------------------------------------------------------------------------------------------------------------------------
int launch_gemm_bias_act(const GemmSegs& S, long M, int N, const EpiBiasAct& e, hipStream_t st) {
    Line("launch_gemm_bias_act").s(st).i("M", M).i("N", N).segs(S).p("out", e.out).i("ldo", e.ldo).p("bias", e.bias).i("act", e.act)
        .f("slope", e.slope).i("out_bf16", e.out_bf16);
    return REGT_OK;
}
int launch_gemm_gates(const GemmSegs& S, long M, int N, const EpiGates& e, hipStream_t st, bool save_r) {
    Line("launch_gemm_gates").s(st).i("M", M).i("N", N).i("save_r", save_r).segs(S).p("ZR", e.ZR).p("h", e.h).p("q", e.q).p("bias", e.bias)
        .i("C", e.C).i("q_bf16", e.q_bf16).i("h_bf16", e.h_bf16).i("zr_bf16", e.zr_bf16);
    return REGT_OK;
}
static void dgrad1(const char* name, const GemmSegs& S, long M, int N, const EpiDgrad1& e, hipStream_t st) {
    Line(name).s(st).i("M", M).i("N", N).segs(S).p("h", e.h).p("ZR", e.ZR).p("dOH", e.dOH).p("probs", e.probs).p("dzr", e.dzr).p("dh", e.dh)
        .i("C", e.C).i("T", e.T).i("dzr_bf16", e.dzr_bf16).i("h_bf16", e.h_bf16).i("zr_bf16", e.zr_bf16).i("dh_bf16", e.dh_bf16)
        .p("Ht", e.Ht).p("dhp", e.dhp).p("rowdot", e.rowdot).i("num_nodes", e.num_nodes);
}
int launch_gemm_dgrad1(const GemmSegs& S, long M, int N, const EpiDgrad1& e, hipStream_t st) { dgrad1("launch_gemm_dgrad1", S, M, N, e, st); return REGT_OK; }
int launch_gemm_dgrad1_gen(const GemmSegs& S, long M, int N, const EpiDgrad1& e, hipStream_t st) { dgrad1("launch_gemm_dgrad1_gen", S, M, N, e, st); return REGT_OK; }
int launch_gemm_dgrad2(const GemmSegs& S, long M, int N, const EpiDgrad2& e, hipStream_t st) {
    Line("launch_gemm_dgrad2").s(st).i("M", M).i("N", N).segs(S).p("dh", e.dh).p("h", e.h).i("C", e.C).i("act", e.act).f("slope", e.slope)
        .i("h_bf16", e.h_bf16).i("dh_bf16", e.dh_bf16);
    return REGT_OK;
}
int launch_gemm_mask_add(const GemmSegs& S, long M, int N, const EpiMaskAdd& e, hipStream_t st) {
    Line("launch_gemm_mask_add").s(st).i("M", M).i("N", N).segs(S).p("out", e.out).i("ldo", e.ldo).p("mask", e.mask).i("ldm", e.ldm)
        .p("add", e.add).i("ldadd", e.ldadd);
    return REGT_OK;
}
int launch_gemm_candidate(const CandArgs& a, hipStream_t st, bool save) {
    Line("launch_gemm_candidate").s(st).i("save", save).segs(a.S).i("num_nodes", a.num_nodes).i("T", a.T).i("C", a.C).p("bias", a.bias)
        .p("ZR", a.ZR).p("h", a.h).p("probs", a.probs).p("Ht", a.Ht).p("OH", a.OH).i("act_bf16", a.act_bf16).i("node_sum_rows", a.node_sum_rows);
    return REGT_OK;
}
int launch_wgrad(const WgradArgs& a, hipStream_t st) {
    Line("launch_wgrad").s(st).p("P", a.P).i("ldp", a.ldp).i("Nout", a.Nout).p("Q", a.Q).i("ldq", a.ldq).i("Nin", a.Nin).i("q_relu", a.q_relu)
        .i("M", a.M).i("kchunk", a.kchunk).p("chunk_tab", a.chunk_tab).i("nchunks", a.nchunks).p("slab", a.slab).i("colsum", a.colsum)
        .p("Q2", a.Q2).i("ldq2", a.ldq2).i("nin_split", a.nin_split).i("p_bf16", a.p_bf16).i("q_bf16", a.q_bf16).i("all_csum", a.all_csum);
    g_max_take = std::max(g_max_take, ((long)a.nchunks * wgrad_slab_stride(a) + 63) & ~63L);
    return REGT_OK;
}
int launch_wgrad_reduce_multi(WgradReduceBatch& b, hipStream_t st) {
    Line l("launch_wgrad_reduce_multi");
    l.s(st).i("n", b.n);
    for (int k = 0; k < b.n; ++k) {
        const WgradReduceArgs& r = b.t[k];
        l.i("task", k).p("slab", r.slab).i("nchunks", r.nchunks).i("slab_stride", r.slab_stride).i("elem_offset", r.elem_offset)
            .i("slab_ld", r.slab_ld).i("Nout", r.Nout).i("Nin", r.Nin).p("chunk_group", r.chunk_group).i("ngroups", r.ngroups)
            .i("group_base", r.group_base).p("out", r.out).i("ldo", r.ldo).i("group_stride", r.group_stride).p("colsum_out", r.colsum_out)
            .i("colsum_offset", r.colsum_offset).i("ncolsum", r.ncolsum).i("accumulate", r.accumulate);
    }
    return REGT_OK;
}
int launch_small_gemm_multi(SgBatch& b, hipStream_t st) {
    Line l("launch_small_gemm_multi");
    l.s(st).i("ntask", b.ntask).i("overflow", b.overflow);
    for (int k = 0; k < b.ntask; ++k) {
        const SgTask& t = b.task[k];
        l.i("task", k).p("C", t.C).p("init", t.init).i("sci", t.sci).i("scj", t.scj).i("scb", t.scb).i("init_si", t.init_si)
            .i("init_sj", t.init_sj).i("m", t.m).i("n", t.n).i("nbatch", t.nbatch).i("nterm", t.nterm);
        for (int j = 0; j < t.nterm; ++j) {
            const SgTerm& q = t.term[j];
            l.i("term", j).p("A", q.A).p("B", q.B).i("sai", q.sai).i("sak", q.sak).i("sab", q.sab).i("sbk", q.sbk).i("sbj", q.sbj)
                .i("sbb", q.sbb).i("k", q.k).i("batch", q.batch).i("sum_batch", q.sum_batch);
        }
    }
    return REGT_OK;
}
int launch_pack_x(const float* x, float* xp, int N, int F, int T, hipStream_t st) {
    Line("launch_pack_x").s(st).p("x", x).p("xp", xp).i("N", N).i("F", F).i("T", T);
    return REGT_OK;
}
int launch_pack_x_bf16(const float* x, void* xp, int N, int F, int T, hipStream_t st) {
    Line("launch_pack_x_bf16").s(st).p("x", x).p("xp", xp).i("N", N).i("F", F).i("T", T);
    return REGT_OK;
}
int launch_cvt_rows_bf16(const float* src, void* dst, long n, hipStream_t st) {
    Line("launch_cvt_rows_bf16").s(st).p("src", src).p("dst", dst).i("n", n);
    return REGT_OK;
}
int launch_spmm_csr(const int* rowptr, const int* col, const float* val, const float* X, float* Y, int nrows, int nrows_x, int W, int nstack,
                    hipStream_t st) {
    Line("launch_spmm_csr").s(st).p("rowptr", rowptr).p("col", col).p("val", val).p("X", X).p("Y", Y).i("nrows", nrows).i("nrows_x", nrows_x)
        .i("W", W).i("nstack", nstack);
    return REGT_OK;
}
int launch_spmm_dual_x(const int* rowptr, const int* col, const float* val_a, const float* val_l, const float* X, float* YA, float* YL,
                       int nnodes, int x_rows, int W, hipStream_t st) {
    Line("launch_spmm_dual_x").s(st).p("rowptr", rowptr).p("col", col).p("val_a", val_a).p("val_l", val_l).p("X", X).p("YA", YA).p("YL", YL)
        .i("nnodes", nnodes).i("x_rows", x_rows).i("W", W);
    return REGT_OK;
}
int launch_spmm_dual_bf16(const int* rowptr, const int* col, const float* val_a, const float* val_l, const void* X, void* YA, void* YL,
                          int nnodes, int x_rows, int W, hipStream_t st) {
    Line("launch_spmm_dual_bf16").s(st).p("rowptr", rowptr).p("col", col).p("val_a", val_a).p("val_l", val_l).p("X", X).p("YA", YA).p("YL", YL)
        .i("nnodes", nnodes).i("x_rows", x_rows).i("W", W);
    return REGT_OK;
}
static void fused_fwd(const char* name, const FusedFwdArgs& a, int C, int F, int waves, hipStream_t st, bool save) {
    Line(name).s(st).i("C", C).i("F", F).i("waves", waves).i("save", save).p("X", a.X).p("LX", a.LX).p("AX", a.AX).p("A0f", a.A0f)
        .p("Aallf", a.Aallf).i("ar_stride", a.ar_stride).p("Uzf", a.Uzf).p("Urf", a.Urf).p("Uhf", a.Uhf).p("Gzrf", a.Gzrf).p("Ghf", a.Ghf)
        .p("bprime", a.bprime).p("czr", a.czr).p("ch", a.ch).p("probs", a.probs).p("node_region", a.node_region).p("h", a.h).p("ZR", a.ZR)
        .p("q", a.q).p("Ht", a.Ht).p("OH", a.OH).i("M", a.M).i("T", a.T).f("slope", a.slope).i("act_lrelu", a.act_lrelu)
        .p("tile_ctr", a.tile_ctr).i("dbg", a.dbg).p("trace", a.trace);
}
int launch_fused_forward(const FusedFwdArgs& a, int C, int F, hipStream_t st, bool save) { fused_fwd("launch_fused_forward", a, C, F, 0, st, save); return REGT_OK; }
int launch_fused_forward_rows(const FusedFwdArgs& a, int C, int F, int waves, hipStream_t st, bool save) {
    fused_fwd("launch_fused_forward_rows", a, C, F, waves, st, save);
    return REGT_OK;
}
int launch_fused_backward(const FusedBwdArgs& a, int C, hipStream_t st) {
    Line("launch_fused_backward").s(st).i("C", C).p("ZR", a.ZR).p("h", a.h).p("Ht", a.Ht).p("dOH", a.dOH).p("probs", a.probs).p("UhTf", a.UhTf)
        .p("UzTf", a.UzTf).p("UrTf", a.UrTf).p("dhp", a.dhp).p("dzr", a.dzr).p("dh", a.dh).p("rowdot", a.rowdot).p("tile_ctr", a.tile_ctr)
        .i("M", a.M).i("T", a.T).f("slope", a.slope).i("act_lrelu", a.act_lrelu).p("trace", a.trace);
    return REGT_OK;
}
int launch_rowdot_reduce(const float* rowdot, float* dp_partial, int num_nodes, int T, int nodes_per_block, hipStream_t st, int parts) {
    Line("launch_rowdot_reduce").s(st).p("rowdot", rowdot).p("dp_partial", dp_partial).i("num_nodes", num_nodes).i("T", T)
        .i("nodes_per_block", nodes_per_block).i("parts", parts);
    return REGT_OK;
}
int launch_cvt_bf16_frag(CvtBatch& b, hipStream_t st) {
    Line l("launch_cvt_bf16_frag");
    l.s(st).i("n", b.n);
    for (int k = 0; k < b.n; ++k) l.i("task", k).p("src", b.t[k].src).i("ld", b.t[k].ld).i("rows", b.t[k].rows).i("cols", b.t[k].cols).p("dst", b.t[k].dst);
    return REGT_OK;
}
int launch_transpose3(const float* s0, const float* s1, const float* s2, int count, float* dst, int rows, int cols, long ld, hipStream_t st) {
    Line("launch_transpose3").s(st).p("s0", s0).p("s1", s1).p("s2", s2).i("count", count).p("dst", dst).i("rows", rows).i("cols", cols).i("ld", ld);
    return REGT_OK;
}
int launch_head2_fwd(const float* y1, const float* W2, const float* b2, float* pred, int N, int H1, int O, hipStream_t st) {
    Line("launch_head2_fwd").s(st).p("y1", y1).p("W2", W2).p("b2", b2).p("pred", pred).i("N", N).i("H1", H1).i("O", O);
    return REGT_OK;
}
int launch_head2_bwd(const float* dpred, const float* W2, const float* y1, float* d1, int N, int H1, int O, hipStream_t st) {
    Line("launch_head2_bwd").s(st).p("dpred", dpred).p("W2", W2).p("y1", y1).p("d1", d1).i("N", N).i("H1", H1).i("O", O);
    return REGT_OK;
}
int launch_head2_wgrad(const float* dpred, const float* y1, float* slab, int N, int H1, int O, int kchunk, int nchunks, int colsum, hipStream_t st) {
    Line("launch_head2_wgrad").s(st).p("dpred", dpred).p("y1", y1).p("slab", slab).i("N", N).i("H1", H1).i("O", O).i("kchunk", kchunk)
        .i("nchunks", nchunks).i("colsum", colsum);
    g_max_take = std::max(g_max_take, ((long)nchunks * ((long)O * H1 + O) + 63) & ~63L);
    return REGT_OK;
}
int launch_sum_region_blocks(const float* W, float* S, int C, int R, hipStream_t st) {
    Line("launch_sum_region_blocks").s(st).p("W", W).p("S", S).i("C", C).i("R", R);
    return REGT_OK;
}
int launch_softmax_small(const float* att, float* probs, int T, hipStream_t st) {
    Line("launch_softmax_small").s(st).p("att", att).p("probs", probs).i("T", T);
    return REGT_OK;
}
int launch_cell_bwd(const CellBwdArgs& a, hipStream_t st) {
    Line("launch_cell_bwd").s(st).p("dOH", a.dOH).p("probs", a.probs).p("ZR", a.ZR).p("h", a.h).p("Ht", a.Ht).p("dhp", a.dhp).p("dzr", a.dzr)
        .p("dp_partial", a.dp_partial).i("num_nodes", a.num_nodes).i("T", a.T).i("C", a.C).i("nodes_per_block", a.nodes_per_block)
        .i("ldz", a.ldz).i("lddz", a.lddz).i("out_bf16", a.out_bf16).i("in_bf16", a.in_bf16);
    return REGT_OK;
}
int launch_att_bwd(const float* dp_partial, int nblocks, const float* probs, float* datt, int T, hipStream_t st) {
    Line("launch_att_bwd").s(st).p("dp_partial", dp_partial).i("nblocks", nblocks).p("probs", probs).p("datt", datt).i("T", T);
    return REGT_OK;
}
int launch_zero_f32(float* dst, long n, hipStream_t st) {
    Line("launch_zero_f32").s(st).p("dst", dst).i("n", n);
    return REGT_OK;
}
int launch_embed_fp32(const float* X, const float* LX, const float* A0, const float* Aall, const int* node_region, const float* bias, float* out,
                      long M, int T, int act, float slope, hipStream_t st) {
    Line("launch_embed_fp32").s(st).p("X", X).p("LX", LX).p("A0", A0).p("Aall", Aall).p("node_region", node_region).p("bias", bias).p("out", out)
        .i("M", M).i("T", T).i("act", act).f("slope", slope);
    return REGT_OK;
}

}  // namespace regt

namespace {
using namespace regt;

// ---- one case: forward, then backward, as api_model.hip calls them -------------------------------------------------------------------------
struct Run { std::vector<Rec> log; std::set<std::string> stages; int rc_fwd = 0, rc_bwd = 0; bool has_bwd = true; size_t fwd_len = 0; };

Run run_case(const Case& c, long slab_floats) {
    g_case = c;
    g_arenas.clear(); g_log.clear(); g_open.clear(); g_event_stream.clear(); g_prof.clear(); g_max_take = 0;
    t_call_flags = c.flags;
    regt_dims d{};
    d.N = c.N; d.T = c.T; d.F = c.F; d.C = c.C; d.R = c.R; d.O = c.O; d.H1 = c.H1; d.regional = c.regional; d.lrelu_slope = 0.01f; d.flags = c.flags;
    char* ws = reinterpret_cast<char*>(arena("ws"));
    regt_graph g{};
    g.rowptr = reinterpret_cast<const int*>(arena("g.rowptr")); g.col = reinterpret_cast<const int*>(arena("g.col")); g.val = arena("g.val");
    if (!c.cell) {
        g.node_region = reinterpret_cast<const int*>(arena("g.node_region"));
        g.chunk_tab = reinterpret_cast<const int*>(arena("g.chunk_tab")); g.chunk_region = reinterpret_cast<const int*>(arena("g.chunk_region"));
        g.n_chunks = 7;
        g.m_rowptr = reinterpret_cast<const int*>(arena("g.m_rowptr")); g.m_col = reinterpret_cast<const int*>(arena("g.m_col"));
        g.m_val_a = arena("g.m_val_a"); g.m_val_l = arena("g.m_val_l");
        g.overlap = c.overlap; g.region_lo = c.region_lo; g.region_hi = c.region_hi; g.region_sorted = c.sorted;
    }
    regt_params p{};
    regt_grads gr{};
    p.attention = arena("p.attention"); gr.attention = c.attention ? arena("g.attention") : nullptr;
    static const char* const KN[3] = {"z", "r", "h"};
    for (int k = 0; k < 3; ++k) {
        const std::string s = KN[k];
        p.conv_lin_w[k] = arena(("p.conv_lin_w_" + s).c_str()); gr.conv_lin_w[k] = arena(("g.conv_lin_w_" + s).c_str());
        p.conv_bias[k] = arena(("p.conv_bias_" + s).c_str()); gr.conv_bias[k] = arena(("g.conv_bias_" + s).c_str());
        p.gate_w[k] = arena(("p.gate_w_" + s).c_str()); gr.gate_w[k] = arena(("g.gate_w_" + s).c_str());
        p.gate_b[k] = arena(("p.gate_b_" + s).c_str()); gr.gate_b[k] = arena(("g.gate_b_" + s).c_str());
    }
    if (!c.cell) {
        p.cheb_w0 = arena("p.cheb_w0"); gr.cheb_w0 = arena("g.cheb_w0");
        p.cheb_w1 = arena("p.cheb_w1"); gr.cheb_w1 = arena("g.cheb_w1");
        p.cheb_bias = arena("p.cheb_bias"); gr.cheb_bias = arena("g.cheb_bias");
    }
    if (c.regional) {
        p.region_w = arena("p.region_w"); gr.region_w = arena("g.region_w");
        p.region_b = arena("p.region_b"); gr.region_b = arena("g.region_b");
    }
    p.head1_w = arena("p.head1_w"); gr.head1_w = arena("g.head1_w");
    p.head1_b = arena("p.head1_b"); gr.head1_b = arena("g.head1_b");
    p.head2_w = arena("p.head2_w"); gr.head2_w = arena("g.head2_w");
    p.head2_b = arena("p.head2_b"); gr.head2_b = arena("g.head2_b");
    const float* x = arena("x");
    const float* xp_ext = c.caller_bf16 ? arena("x_packed_bf16") : nullptr;
    const int x_rows = c.caller_bf16 ? c.N + 8 : 0;
    float *pred = arena("pred"), *hidden = arena("hidden");
    const float *dpred = arena("dpred"), *dhidden = arena("dhidden");
    const float* h_ext = c.cell ? arena("h_in") : nullptr;
    float* dh_ext = c.cell ? arena("dh_in") : nullptr;

    Run r;
    int fmt = c.cell ? (bf16_intermediates(d) ? FMT_QBF : 0) : forward_format(d, g, xp_ext ? x_rows : d.N, false, c.caller_bf16);
    Layout L;
    if (c.fwd_only) {
        L = c.cell ? make_layout_fwd(d, 0, false, d.N, ws) : forward_only_layout(d, g, xp_ext != nullptr, x_rows, c.caller_bf16, ws, &fmt);
        fmt |= FMT_FWDONLY;
    } else {
        L = make_layout(d, g.n_chunks, g.overlap, ws);
    }
    { Line l("forward"); l.i("fmt", fmt); }
    r.rc_fwd = forward_impl(d, g, p, c.caller_bf16 ? nullptr : x, xp_ext, x_rows, pred, hidden, L, MAIN, false, h_ext, fmt);
    r.fwd_len = g_log.size();
    r.has_bwd = !c.fwd_only;
    if (r.has_bwd) {
        if (slab_floats > 0) L.slab_floats = slab_floats;
        { Line l("backward"); l.i("fmt", fmt).i("slab_floats", L.slab_floats); }
        r.rc_bwd = backward_impl(d, g, p, gr, dpred, dhidden, hidden, xp_ext, L, MAIN, fmt, h_ext, dh_ext);
    }
    // resolve the PROF scopes of every launch: g_prof holds name and first event of each scope that has closed
    std::vector<std::string> scope_name(g_event_stream.size());
    for (const ProfRec& pr : g_prof) {
        const int id = (int)reinterpret_cast<unsigned long long>(pr.e0) - 1;
        scope_name[id] = std::string(pr.name) + "@" + stream_name(g_event_stream[id]);
        r.stages.insert(pr.name);
    }
    for (Rec& rec : g_log) {
        std::string s;
        for (int id : rec.scopes) s += (s.empty() ? "" : ",") + scope_name[id];
        rec.text = " prof=" + (s.empty() ? std::string("-") : s) + rec.text;
    }
    r.log = g_log;
    return r;
}

std::vector<Case> all_cases() {
    std::vector<Case> v;
    auto add = [&](const char* name, Case c) { c.name = name; v.push_back(c); };
    const Case c1;                                                        // 1: regional fp32, R = 5, F = 32, sorted region ids
    add("01_regional_fp32", c1);
    { Case c = c1; c.F = 8; add("02_F8", c); }
    { Case c = c1; c.R = 1; add("03_R1", c); }
    Case c4 = c1; c4.overlap = 1;
    add("04_overlap", c4);
    { Case c = c1; c.region_lo = 1; c.region_hi = 3; add("05_shard_1_3", c); }
    { Case c = c1; c.O = 8; add("06_O8", c); }
    { Case c = c1; c.attention = false; add("07_no_attention_grad", c); }
    { Case c = c1; c.opt[OPT_DGRAD1_GEN] = 0; add("08_no_dgrad1_gen", c); }
    { Case c = c1; c.wide = true; add("09_fp32_core_wide", c); }
    { Case c = c1; c.mode = 1; add("10_bf16x3", c); }
    Case c11 = c1; c11.regional = 0; c11.R = 1;
    add("11_tgcn_collapsed_F32", c11);
    { Case c = c11; c.F = 8; add("12_tgcn_collapsed_F8", c); }
    { Case c = c11; c.opt[OPT_TGCN_COLLAPSE] = 0; add("13_tgcn_uncollapsed", c); }
    Case c14 = c1; c14.mode = 2; c14.F = 64;
    add("14_bf16_fused", c14);
    { Case c = c14; c.flags |= REGT_DIMS_NO_FUSED_BWD; c.opt[OPT_WGRAD_PAIRS] = 0; c.opt[OPT_FUSED_ROWS] = 0; add("15_bf16_three_launch_bwd", c); }
    { Case c = c14; c.flags |= REGT_DIMS_NO_BF16_ROWS; add("16_bf16_no_bf16_rows", c); }
    { Case c = c14; c.caller_bf16 = true; add("17_bf16_caller_rows", c); }
    { Case c = c1; c.cell = true; c.regional = 0; c.R = 1; add("18_cell", c); }
    { Case c = c1; c.fwd_only = true; c.flags |= REGT_DIMS_FORWARD_ONLY; add("19_forward_only", c); }
    { Case c = c4; c.min_slab = true; add("20_overlap_min_slab", c); }
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    const bool full = argc > 1 && !strcmp(argv[1], "--full");
    std::set<std::string> stages;
    for (const Case& c : all_cases()) {
        long slab = 0;
        if (c.min_slab) { run_case(c, 0); slab = g_max_take; }      // a first pass finds the largest single request
        const Run r = run_case(c, slab);
        printf("case %s rc %d %d launches %zu\n", c.name, r.rc_fwd, r.rc_bwd, r.log.size());
        for (size_t k = 0; k < r.log.size(); ++k) {
            const Rec& rec = r.log[k];
            if (full) printf("%s %03zu %s%s\n", k < r.fwd_len ? "fwd" : "bwd", k, rec.name.c_str(), rec.text.c_str());
            else printf("%s %03zu %s %016llx\n", k < r.fwd_len ? "fwd" : "bwd", k, rec.name.c_str(), fnv1a(rec.name + rec.text));
        }
        stages.insert(r.stages.begin(), r.stages.end());
    }
    printf("stages");
    for (const std::string& s : stages) printf(" %s", s.c_str());
    printf("\n");
    return 0;
}
