// Internal C++ launcher interface of the regtgcn HIP library (not exported; see include/regtgcn.h
// for the C ABI).  Every launcher enqueues on the given stream and returns REGT_OK / error code.
#pragma once
#include <atomic>

#include "gemm_core.h"
#include "options.h"

namespace regt {
// developer build (-DREGT_WG_TRACE, tools/wg_trace.py): per-workgroup wall-clock marks inside the GEMM cores
#ifdef REGT_WG_TRACE
#ifndef REGT_WG_TRACE_N
#define REGT_WG_TRACE_N 512
#endif
constexpr int WG_TRACE_MAX = 40000;
extern __device__ long g_wg_marks[8 * WG_TRACE_MAX];
// id of the tile at hand: wherever the macros are used, rm / n0 / N name the tile
#define WG_TILE_ID ((int)(rm.base / 128) * ((N + 127) / 128) + n0 / 128)
#define WG_MARK(i) do { if (threadIdx.x == 0 && WG_TILE_ID < WG_TRACE_MAX && N == REGT_WG_TRACE_N) g_wg_marks[8L * WG_TILE_ID + (i)] = wall_clock64(); } while (0)
#else
#define WG_MARK(i) do { } while (0)
#endif

// ---- buffer-descriptor addressing for the straight-line epilogues (functors of gemm_fwd.hip / gemm_cell.hip) ----------------------------------
// One descriptor per array and tile (its base is the tile's origin, wave-uniform), a per-thread byte offset and a
// wave-uniform scalar offset per row slot: no vector instruction is spent on addresses inside the row loops.
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_srd(const void* p) {      // p must be wave-uniform
    const unsigned long long a = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0, 0x7FFFFFF0, 0x00020000);
}
__device__ __forceinline__ float4 buf_ld4(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ void buf_st4(__amdgpu_buffer_rsrc_t r, int voff, int soff, float4 v) {
    const u32x4_t w = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(w, r, voff, soff, 0);
}
// four fp32 -> four bf16 (round to nearest even), one 8-byte store
__device__ __forceinline__ void buf_st4_bf16(__amdgpu_buffer_rsrc_t r, int voff, int soff, float4 v) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t lo = {v.x, v.y}, hi = {v.z, v.w};
    const u32x2_t w = {__builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf16x2_t)),
                       __builtin_bit_cast(unsigned, __builtin_convertvector(hi, bf16x2_t))};
    __builtin_amdgcn_raw_buffer_store_b64(w, r, voff, soff, 0);
}
// GRU blend H' = Z h + (1 - Z) H~ (models/utils.py:186-188) with ONE fixed instruction sequence -- fma(Z, h, fl((1 - Z) H~)) --
// wherever it is computed (candidate epilogues in gemm_cell.hip, fused forward in fused.hip): left to -ffp-contract the two
// kernels could round differently, and tests/test_gpu_fused.py compares them bit for bit.
__device__ __forceinline__ float gru_blend(float Z, float h, float ht) { return fmaf(Z, h, __fmul_rn(1.0f - Z, ht)); }
// The element-wise steps of the cell's backward pass, likewise with one fixed instruction sequence each (cell_bwd8_kernel and the
// data-gradient epilogues of the three-launch path, the fused backward kernel in fused.hip):  with g = p_t dOH[node]
//   dhp = g (1 - Z) (1 - H~^2)        dzp = g (h - H~) Z (1 - Z)        drp = dq h R (1 - R)        dh = dq R + g Z
//   ds = (dh + dzp Uz + drp Ur) act'(h)
__device__ __forceinline__ float cb_dhp(float g, float z, float ht) { return __fmul_rn(__fmul_rn(g, 1.0f - z), fmaf(-ht, ht, 1.0f)); }
__device__ __forceinline__ float cb_dzp(float g, float h, float ht, float z) { return __fmul_rn(__fmul_rn(g, h - ht), __fmul_rn(z, 1.0f - z)); }
__device__ __forceinline__ float cb_drp(float dq, float h, float r) { return __fmul_rn(__fmul_rn(dq, h), __fmul_rn(r, 1.0f - r)); }
__device__ __forceinline__ float cb_dh(float dq, float r, float p, float d, float z) { return fmaf(dq, r, __fmul_rn(__fmul_rn(p, d), z)); }
__device__ __forceinline__ float cb_ds(float dh, float acc, float factor) { return __fmul_rn(dh + acc, factor); }

// per tile row: byte offset of the row's node in an (N, C) fp32 array and its period's attention probability (EpiDgrad1F)
struct EpiRowEnt { int off; float p; };
// where a thread sits in the epilogue of a full tile: rows rr + step * i (i = row slot), columns c .. of the tile at (m0, n0)
struct EpiGeom { long m0; int n0, rr, c, step; const EpiRowEnt* rowtab; };
constexpr int EPI_ROWTAB_BYTES = 128 * (int)sizeof(EpiRowEnt);


// ---- epilogue descriptors for the flat segmented GEMM ------------------------------------------
enum : int { ACT_NONE = 0, ACT_LRELU = 1, ACT_RELU = 2, ACT_SIGMOID = 3, ACT_TANH = 4 };

// `*_bf16` flags (REGT_GEMM_MODE=bf16 with bf16 storage of the M x C activations): the array holds bf16 elements (strides
// in elements); the bf16-operand core then runs its 8-column-per-thread epilogue so that every access stays 16 bytes wide.
struct EpiBiasAct {     // out[m, c] = act(v + bias[c])
    float* out; long ldo; const float* bias; int act; float slope;
    int out_bf16 = 0;
};
struct EpiGates {       // N = 2C: c <  C: Z = sigmoid(v + b) -> ZR[m, c]
    float* ZR;          //         c >= C: R = sigmoid(v + b) -> ZR[m, c], q[m, c-C] = h[m, c-C] * R
    const float* h; float* q; const float* bias; int C;
    int q_bf16 = 0;     // q is stored as bf16 (row stride C elements): it only ever feeds matrix-core operands
    int h_bf16 = 0, zr_bf16 = 0;
};
struct EpiDgrad1 {      // v = dq[m, c]:  dzr[m, C+c] = v*h*R*(1-R);  dh[m, c] = v*R + p[t]*dOH[node, c]*Z
    const float* h; const float* ZR; const float* dOH; const float* probs;
    float* dzr; float* dh; int C; int T;
    int dzr_bf16 = 0;   // dzr is stored as bf16 (row stride 2C elements)
    int h_bf16 = 0, zr_bf16 = 0, dh_bf16 = 0;
    // launch_gemm_dgrad1_gen (fp32): the left operand dhp = g (1 - Z)(1 - H~^2) is GENERATED from Z, H~, dOH while it is staged (and
    // stored to dhp for the weight gradients); the epilogue also writes dzp = g (h - H~) Z (1 - Z) -> dzr[m, c] and the row's
    // partial attention dot <dOH, Z h + (1 - Z) H~> over the tile's 128 columns -> rowdot[m * (C / 128) + c / 128]
    const float* Ht = nullptr; float* dhp = nullptr; float* rowdot = nullptr; int num_nodes = 0;
};
struct EpiDgrad2 {      // ds[m, c] = (dh[m, c] + v) * act'(h[m, c])   (in place on dh)
    float* dh; const float* h; int C; int act; float slope;
    int h_bf16 = 0, dh_bf16 = 0;
};
struct EpiMaskAdd {     // out[m, c] = v * (mask[m, c] > 0) + (add ? add[m, c] : 0)
    float* out; long ldo; const float* mask; long ldm; const float* add; long ldadd;
};

int launch_gemm_bias_act(const GemmSegs& S, long M, int N, const EpiBiasAct& e, hipStream_t st);
// save_r = false (forward-only calls): the R half of ZR is not written (Z and q are)
int launch_gemm_gates(const GemmSegs& S, long M, int N, const EpiGates& e, hipStream_t st, bool save_r = true);
int launch_gemm_dgrad1(const GemmSegs& S, long M, int N, const EpiDgrad1& e, hipStream_t st);
// cell_bwd + dgrad_candidate in one launch (fp32 arithmetic, C % 128 == 0, big-tile regime): see EpiDgrad1's last fields
bool gemm_dgrad1_gen_ok(long M, int C, int num_nodes);
bool wgrad_ring_chunking(int Nout, int Nin, long M, int* kchunk, int* nchunks);
bool wgrad_skinny_chunking(int Nout, long M, int* kchunk, int* nchunks);            // skinny (Nin <= 32) fp32-MFMA kernel
bool wgrad_wide_chunking(int Nout, int Nin, long M, int* kchunk, int* nchunks);   // wide fp32 / bf16x3 kernels (experiment)
// wave-owned fp32 kernel (wgrad_wave_kernel): whether a gradient has its shape under the current switches, its chunks (one per CU;
// wgrad_wide_chunking returns them where they apply), and the smallest M it is chosen for
bool wgrad_wave_shape(int Nout, int Nin);
bool wgrad_wave_chunking(int Nout, long M, int* kchunk, int* nchunks);
long wgrad_wave_min_rows();
long wgrad_chunk_bound(int Nout, int Nin, long M);   // upper bound of what the three can return (slab sizing, api_layout.hip make_layout)
bool wgrad_ring_active();             // the ring kernel takes the bf16-stored weight gradients (pairs pay off with it)
int launch_gemm_dgrad1_gen(const GemmSegs& S, long M, int N, const EpiDgrad1& e, hipStream_t st);
int launch_gemm_dgrad2(const GemmSegs& S, long M, int N, const EpiDgrad2& e, hipStream_t st);
int launch_gemm_mask_add(const GemmSegs& S, long M, int N, const EpiMaskAdd& e, hipStream_t st);

// Candidate-state GEMM with the loop over the T periods inside the workgroup:
//   for t: Ht = tanh(q_t Uh2^T + ax_t Gh^T + ch);  Hn = Z*h + (1-Z)*Ht;  OH += p[t]*Hn
struct CandArgs {
    GemmSegs S;             // segments with A rows addressed as (node*T + t)
    int num_nodes, T, C;
    const float* bias;      // ch (C)
    const float* ZR;        // (M, 2C)
    const float* h;         // (M, C)
    const float* probs;     // (T)
    float* Ht;              // (M, C) out
    float* OH;              // (num_nodes, C) out
    int act_bf16 = 0;       // ZR, h and Ht hold bf16 elements (all three together)
    int node_sum_rows = 64; // bf16 storage: the rows of a node are summed in row order inside blocks of 64 (the staged half) or 16
                            //   rows (what a wave of fused_rows.hip owns: the two paths then agree bit for bit); T <= 16 for the latter
};
// save = false (forward-only calls): H~ is not stored, a.Ht may be NULL
int launch_gemm_candidate(const CandArgs& a, hipStream_t st, bool save = true);

// ---- weight-gradient GEMM: out[Nout x Nin] = P^T Q, split over row chunks ----------------------
struct WgradArgs {
    const float* P; long ldp; int Nout;
    const float* Q; long ldq; int Nin;
    int q_relu;               // apply relu to Q while staging
    long M;                   // rows
    int kchunk;               // rows per chunk (uniform) when chunk_tab == nullptr
    const int* chunk_tab;     // optional (nchunks, 2) [row_start, row_end)
    int nchunks;
    float* slab;              // (nchunks, Nout*Nin + (colsum ? Nout : 0))
    int colsum;               // also produce column sums of P (bias gradient)
    // optional second right-hand operand (skinny kernel only): output columns >= nin_split come from Q2 (column j -
    // nin_split).  Two gradients that share P -- dA0 = ds^T x and dA_r = ds^T (L~ x) -- then read P from HBM once.
    const float* Q2 = nullptr; long ldq2 = 0; int nin_split = 0;
    int p_bf16 = 0, q_bf16 = 0;   // P / Q hold bf16 elements (ldp / ldq in elements); vector kernels only
    int all_csum = 0;             // ring kernel: every column tile forms the column sums (only tile 0 stores them)
};
int launch_wgrad(const WgradArgs& a, hipStream_t st);
long wgrad_slab_stride(const WgradArgs& a);
// Which of the 18 GEMM kernels a weight gradient runs on, with what grid and dynamic LDS: decided by wgrad_pick (wgrad_dispatch.hip,
// launches nothing, makes every refusal), launched by the unit that holds the kernel.
enum WgradKernel : int {
    WG_SKINNY32, WG_SKINNY32_PBF, WG_MID64, WG_WIDE128, WG_WIDE3, WG_GENERIC32, WG_GENERIC128, WG_WAVE,      // wgrad_fp32.hip
    WG_SPLIT3, WG_SPLIT1, WG_SPLIT1_QBF, WG_SPLIT1_PBF, WG_SPLIT1_PBF_QBF,                          // wgrad_bf16.hip (WG_SPLIT1 + 2 p_bf16 + q_bf16)
    WG_RING_4_2, WG_RING_6_2, WG_RING_8_2, WG_RING_2_4, WG_RING_4_4
};
static_assert(WG_SPLIT3 == WG_WAVE + 1, "launch_wgrad: the kernels of wgrad_fp32.hip come first, then those of wgrad_bf16.hip");
static_assert(WG_SPLIT1_QBF == WG_SPLIT1 + 1 && WG_SPLIT1_PBF == WG_SPLIT1 + 2 && WG_SPLIT1_PBF_QBF == WG_SPLIT1 + 3,
              "wgrad_pick: WG_SPLIT1 + 2 p_bf16 + q_bf16");
struct WgradPick { WgradKernel kernel; long blocks; size_t lds; bool raise_lds; };      // raise_lds: the kernel's dynamic-LDS limit is asked for
int wgrad_pick(const WgradArgs& a, WgradPick* p);
int launch_wgrad_slabs(const WgradArgs& a, hipStream_t st, bool any_rows, WgradKernel* ran);     // launch_wgrad, optionally below WG_WAVE's row gate; *ran = the kernel
const char* wgrad_kernel_name(WgradKernel k);
int launch_wgrad_fp32(const WgradPick& p, const WgradArgs& a, hipStream_t st);
int launch_wgrad_bf16(const WgradPick& p, const WgradArgs& a, hipStream_t st);

struct WgradReduceArgs {
    const float* slab; int nchunks; long slab_stride;
    long elem_offset;         // first slab element of the (Nout x Nin) block to reduce
    long slab_ld;             // row stride of that block inside a slab (0: dense, = Nin)
    int Nout, Nin;
    const int* chunk_group;   // optional (nchunks): output group of each chunk
    int ngroups;              // groups group_base .. group_base + ngroups - 1 are reduced (into out blocks 0 .. ngroups - 1)
    int group_base;
    float* out; long ldo; long group_stride;   // out[g*group_stride + i*ldo + j]
    float* colsum_out;        // optional (ncolsum), only ngroups == 1
    long colsum_offset;       // slab element of the first column sum
    int ncolsum;
    int accumulate;           // add into out instead of overwrite
};
int launch_wgrad_reduce(const WgradReduceArgs& a, hipStream_t st);
// several independent reductions in one launch (the backward pass defers all of its slab reductions to one place)
constexpr int WR_MAX_TASKS = 12;
struct WgradReduceBatch {
    int n;
    int block_start[WR_MAX_TASKS + 1];
    WgradReduceArgs t[WR_MAX_TASKS];
};
int launch_wgrad_reduce_multi(WgradReduceBatch& b, hipStream_t st);

// ---- tiny strided batched GEMM (weight composition and its backward) ---------------------------
//   C[b][i, j] (+)= sum_over_batch? sum_k A[b][i, k] * B[b][k, j]      arbitrary strides
struct SmallGemm {
    const float* A; long sai, sak, sab;
    const float* B; long sbk, sbj, sbb;
    float* C; long sci, scj, scb;
    int m, n, k, batch;
    int sum_batch;     // 1: reduce over the batch index into one C
    int accumulate;    // 1: C += result
};
int launch_small_gemm(const SmallGemm& g, hipStream_t st);

// Several such products in ONE launch (the per-step weight compositions are ~27 tiny dependent-free GEMMs; one
// launch each would dominate the step at TPIMS size).  out[b][i,j] = init[i] + sum_terms sum_k A[..]*B[..].
// (compact: 32-bit strides, 16-bit counts -- a whole batch is passed BY VALUE in the kernel-argument block, 4 KB at most, and the
// composition backward is one launch of 19 tasks since round 4)
struct SgTerm {                  // 48 bytes
    const float* A; const float* B;
    int sai, sak, sab, sbk, sbj, sbb;
    int k;                       // sum length (< 0: a stride did not fit 32 bits -- add_task refuses the task)
    short batch, sum_batch;      // sum_batch: reduce over `batch` operand pairs; else use the output's batch index
};
struct SgTask {                  // 200 bytes
    float* C; const float* init; // optional init[i*init_si + j*init_sj] added to the sum (nullptr: 0; init_sj = 0: the same value
    int sci, scj, scb, init_si, init_sj;   // for every column)
    int m, n;                    // output (nbatch, m, n)
    short nbatch, nterm;
    short split, pad_;           // lanes per output element (set by launch_small_gemm_multi: 1 for short sums, 8 for long ones, 0 tiled)
    SgTerm term[3];
};
constexpr int SG_MAX_TASKS = 19;
struct SgBatch {
    int ntask;
    int overflow;                // set by add_task when a task did not fit (launch_small_gemm_multi then fails)
    int block_start[SG_MAX_TASKS + 1];
    SgTask task[SG_MAX_TASKS];
};
static_assert(sizeof(SgBatch) <= 4000, "SgBatch travels in the kernel-argument block");
int launch_small_gemm_multi(SgBatch& b, hipStream_t st);

// ---- graph preparation (graph.hip) ---------------------------------------------------------------
size_t graph_workspace_bytes(long E, int N);
int graph_gcn_csr(const int64_t* ei, const float* w, long E, int N, int* rowptr, int* col, float* val,
                  int* flags_out_dev, void* ws, size_t ws_bytes, hipStream_t st);
int graph_gcn_dis(const int64_t* ei, const float* w, long E, int N, float* dis_out, int* flags_out_dev, void* ws, size_t ws_bytes,
                  hipStream_t st);
int graph_cheb_edge_weights(const int64_t* ei, const float* w, long E, int N, float* out_w, int* flags_out_dev,
                            void* ws, size_t ws_bytes, hipStream_t st);
int graph_raw_csr(const int64_t* ei, const float* w, long E, int N, int* rowptr, int* col, float* val,
                  int* flags_out_dev, void* ws, size_t ws_bytes, hipStream_t st);
int graph_fingerprint(const int64_t* ei, const float* w, long E, unsigned long long* out_dev, hipStream_t st);
int graph_mean_csr(const int64_t* ei, long E, int N, int* rowptr, int* col, float* val, int* flags_out_dev, void* ws,
                   size_t ws_bytes, hipStream_t st);

// ---- sparse aggregation ------------------------------------------------------------------------
int launch_pack_x(const float* x, float* xp, int N, int F, int T, hipStream_t st);            // (N,F,T) -> (N,T,F)
int launch_spmm_csr(const int* rowptr, const int* col, const float* val, const float* X, float* Y,
                    int nrows, int nrows_x, int W, int nstack, hipStream_t st);                  // Y[r] = sum val*X[col]; rows = nstack x nodes

int launch_spmm_dual(const int* rowptr, const int* col, const float* val_a, const float* val_l, const float* X, float* YA,
                     float* YL, int nnodes, int W, hipStream_t st);   // YA = A x, YL = L x from one merged CSR (two weights/entry)
// the same with X holding x_rows >= nnodes rows (region shard: own rows, then halo rows)
int launch_spmm_dual_x(const int* rowptr, const int* col, const float* val_a, const float* val_l, const float* X, float* YA,
                       float* YL, int nnodes, int x_rows, int W, hipStream_t st);
// bf16 rows in (X: x_rows x W bf16) and out (YA, YL: nnodes x W bf16), fp32 accumulation, one rounding at the end; W % 64 == 0
int launch_spmm_dual_bf16(const int* rowptr, const int* col, const float* val_a, const float* val_l, const void* X, void* YA, void* YL,
                          int nnodes, int x_rows, int W, hipStream_t st);

int launch_pack_x_bf16(const float* x, void* xp, int N, int F, int T, hipStream_t st);        // (N,F,T) fp32 -> (N,T,F) bf16, F % 8 == 0
int launch_cvt_rows_bf16(const float* src, void* dst, long n, hipStream_t st);                // n % 8 == 0 elements fp32 -> bf16

// ---- fused forward of the cell for the bf16 arithmetic (fused.hip) ----------------------------------------------------------
struct FusedFwdArgs {
    const void *X, *LX, *AX;                  // bf16 rows (M x F): packed input, L~ x, A_hat x (rows node * T + t)
    const void *A0f, *Aallf; long ar_stride;  // composed (C x F) weights in MFMA fragment order (launch_cvt_bf16_frag), one block per region
    const void *Uzf, *Urf, *Uhf;              // the h-halves of linear_z / _r / _h (C x C), fragment order
    const void *Gzrf, *Ghf;                   // composed [Gz; Gr] (2C x F) and Gh (C x F), fragment order
    const float *bprime, *czr, *ch, *probs;   // composed biases (C, 2C, C), softmax(attention) (T)
    const int* node_region;                   // (nodes) or nullptr (one region)
    void *h, *ZR, *q, *Ht;                    // bf16 outputs: (M x C), (M x 2C) = [Z | R], (M x C), (M x C); not touched (may be NULL) with save = false
    float* OH;                                // (nodes x C) fp32, zero-initialised: the attention-weighted hidden state
    long M; int T; float slope; int act_lrelu;
    long nodes;                               // M / T                                            } filled in by launch_fused_forward
    unsigned long long pmask;                 // bit k T for every k T < 64 (rows that start a node) }
    unsigned* tile_ctr;                       // workspace word (zeroed by the launcher): the persistent workgroups draw their tiles from it
    const char* wbase;                        // fused_rows.hip: the weight blocks as 32-bit offsets from one base (filled in by its launcher)
    unsigned o_uz, o_ur, o_uh, o_gzr, o_gh, o_a0, o_aall;
    int dbg;                                  // timing-only switch (REGT_FUSED_DBG, fused.hip: bit 1 = no weight traffic); 0 in normal operation
    long* trace;                              // developer trace buffer (REGT_FUSED_TRACE) or nullptr
};
long fused_trace_fetch(long* out, long capacity);
// save = false: the forward-only instantiation (no activation stores; REGT_DIMS_FORWARD_ONLY)
int launch_fused_forward(const FusedFwdArgs& a, int C, int F, hipStream_t st, bool save = true);
bool fused_forward_ok(int C, int F);
// the row-owning form (fused_rows.hip): a wave owns 16 whole rows, weights stream through LDS; needs region ids sorted by node.
// waves = 8: one workgroup of eight waves per CU (the product form); 4: two workgroups of four with half the ring each (slower --
// twice the weight traffic -- kept because its short ring is the harder test of the hand-counted waits)
int launch_fused_forward_rows(const FusedFwdArgs& a, int C, int F, int waves, hipStream_t st, bool save = true);
bool fused_forward_rows_ok(int C, int F, int T);

// ---- fused data gradients of the cell for the bf16 arithmetic (fused.hip): cell_bwd + dgrad_candidate + dgrad_gates in one kernel
struct FusedBwdArgs {
    const void *ZR, *h, *Ht;                  // bf16, stored by the forward: (M x 2C) = [Z | R], (M x C), (M x C)
    const float *dOH, *probs;                 // (nodes x C) fp32 gradient of the attention-weighted hidden state, softmax(attention) (T)
    const void *UhTf, *UzTf, *UrTf;           // TRANSPOSED h-halves of linear_h / _z / _r (C x C) in MFMA fragment order
    void *dhp, *dzr, *dh;                     // bf16 outputs: (M x C), (M x 2C) = [dzp | drp], (M x C) = ds
    float* rowdot;                            // (M) fp32: <dOH[node], H'[m]> per row (attention-probability gradient, summed later)
    unsigned* tile_ctr;                       // workspace word (zeroed by the launcher): the persistent workgroups draw their tiles from it
    long M; int T; float slope; int act_lrelu;
    long* trace;                              // developer trace buffer (REGT_FUSED_TRACE=2) or nullptr
};
int launch_fused_backward(const FusedBwdArgs& a, int C, hipStream_t st);
bool fused_backward_ok(int C);
// dp_partial[b][t] = sum over the nodes of block b (nodes_per_block consecutive nodes, ascending) of rowdot[node * T + t]
// (`parts` > 1: a row holds `parts` consecutive partial dots, added in ascending order)
int launch_rowdot_reduce(const float* rowdot, float* dp_partial, int num_nodes, int T, int nodes_per_block, hipStream_t st, int parts = 1);

// ---- cell backward head / small element-wise kernels -------------------------------------------
// GEMM arithmetic: 0 = fp32 MFMA (default), 1 = exact 3-way bf16 split on the bf16 MFMA (gemm_split.h)
int gemm_mode();
int gemm_mode_override(int mode);   // thread-local override for one call (-1 = none); returns the previous override
bool fp32_core_wide();   // REGT_FP32_CORE=wide (A/B timing of the two fp32 GEMM cores)

// fp32 -> bf16 (round to nearest even) copies of up to 8 weight blocks in MFMA fragment order (SEG_B_FRAG), one launch:
// block t = rows x cols (cols % 16 == 0) at src with leading dimension ld; dst holds ceil(rows / 128) * 128 rows (zero padded)
struct CvtTask { const float* src; long ld; int rows, cols; void* dst; };
struct CvtBatch { int n; CvtTask t[8]; int block_start[9]; };
int launch_cvt_bf16_frag(CvtBatch& b, hipStream_t st);
inline long frag_bytes(long rows, long cols) { return ((rows + 127) / 128) * 128 * cols * 2; }
bool gemm_desc_table_forced();     // REGT_GEMM_DESC=table
int launch_transpose3(const float* s0, const float* s1, const float* s2, int count, float* dst, int rows, int cols, long ld,
                      hipStream_t st);   // dst[b] = src[b]^T, b < count <= 3
// last head layer for output_dim <= 4 as row-wise fp32 kernels (cell.hip)
bool head2_skinny_ok(int H1, int O, const void* y1, const void* W2);
int launch_head2_fwd(const float* y1, const float* W2, const float* b2, float* pred, int N, int H1, int O, hipStream_t st);
int launch_head2_bwd(const float* dpred, const float* W2, const float* y1, float* d1, int N, int H1, int O, hipStream_t st);
int launch_head2_wgrad(const float* dpred, const float* y1, float* slab, int N, int H1, int O, int kchunk, int nchunks, int colsum,
                       hipStream_t st);
// S[i, j] = sum_r W[i, r*C + j]: the sum of the R (C x C) blocks of tgnn.linear.weight (cell.hip)
int launch_sum_region_blocks(const float* W, float* S, int C, int R, hipStream_t st);
int launch_softmax_small(const float* att, float* probs, int T, hipStream_t st);
// attention-weighted window sum over a ring of per-time-step cell outputs (window.hip): hidden[w] = sum_p probs[p] ring[(first_slot + w + p)
// % ring_len], every element in the order p = 0 .. T - 1 with fmaf from 0.  windows == 1 reads T slabs; more run in chunks of WINDOW_WC
// windows per thread, WINDOW_WC + T - 1 slab reads per chunk.
constexpr int WINDOW_WC = 16;
constexpr int WINDOW_MAX_CHUNKS = 65535;      // chunks of one launch (grid.y): the entry point refuses more windows than that covers
int window_chunk(int windows);      // windows a thread accumulates at once: 1 or WINDOW_WC (regt_window_chunk hands it to tools and tests)
int launch_window_sum(const float* ring, const float* probs, float* hidden, int ring_len, int first_slot, int windows, int N, int T, int C,
                      hipStream_t st);
// Backward of the window sum (window_bwd.hip).  The adjoint: dring[(first_slot + j) % ring_len] (+)= sum_w probs[j - w]
// dhidden[w] over the windows w that contain covered slot j < windows + T - 1, every element from the value dring holds (accumulate) or
// from 0, its windows ascending, one fmaf each; slots are taken in chunks of window_chunk(windows) per thread.  The attention gradient:
// dprob[p] = sum_{w, n, c} dhidden[w] ring[slot(w + p)] in one pass -- per-thread sums, one partial row per workgroup in `partial`
// (window_attgrad_blocks rows of T floats), then one small launch that sums the rows in a fixed order and applies the softmax backward
// into d_attention (added to under `accumulate`, else written).
constexpr int WINDOW_BWD_MAX_T = 32;      // periods the backward covers (the attention gradient keeps one accumulator per period in registers)
int launch_window_adjoint(const float* dhidden, const float* probs, float* dring, int ring_len, int first_slot, int windows, int N, int T,
                          int C, int accumulate, hipStream_t st);
long window_attgrad_blocks(int windows, int N, int C);
int launch_window_attgrad(const float* ring, const float* dhidden, const float* probs, float* partial, float* d_attention, int ring_len,
                          int first_slot, int windows, int N, int T, int C, int accumulate, hipStream_t st);
// dst[k][i] = src[k][i] (+ dst[k][i] under `accumulate`) for up to four vectors in one launch
struct DeliverArgs { const float* src[4]; float* dst[4]; long n[4]; int count; int accumulate; };
int launch_deliver(const DeliverArgs& a, hipStream_t st);
struct CellBwdArgs {
    const float* dOH; const float* probs; const float* ZR; const float* h; const float* Ht;
    float* dhp; float* dzr; float* dp_partial; int num_nodes, T, C; int nodes_per_block;
    // zero-hidden cell (GraphSAGE / GAT models): h == nullptr means H = 0; Z and dzp then are plain (M, C) arrays
    int ldz = 0, lddz = 0;     // row strides of ZR and dzr in floats; 0 = 2C ([Z|R] and [dzp|drp] layouts of the GRU cell)
    int out_bf16 = 0;   // dhp / dzr are stored as bf16 (same element strides)
    int in_bf16 = 0;    // ZR, h and Ht hold bf16 elements (all three together; needs out_bf16 and C % 8 == 0)
};
int launch_cell_bwd(const CellBwdArgs& a, hipStream_t st);
// the cell's input gradient in front of the transposed aggregation (cell_dx.hip): dAx (N, F) = [dzp | drp] [Gz; Gr] + dhp Gh, one pass over
// dzr (N, 2C) and dhp (N, C); C % 4 == 0, F % 4 == 0, F <= 64, 16-byte aligned pointers
int launch_cell_dx(const float* dzr, const float* dhp, const float* Gzr, const float* Gh, float* dAx, int N, int C, int F, hipStream_t st);
// the whole model's input gradient in front of the transposed aggregation (model_dx.hip): three (M, F) outputs from three row segments in one
// pass.  Segment s streams A[s] (M, K[s]) once; B[s][o] (K[s], F) multiplies it into out[o] (NULL: not).  node_region != NULL: B[2][2] is
// ignored and row m takes the block Breg + node_region[m / T] * breg_stride (ids clamped to [0, R)); regions need not be sorted.
struct ModelDxArgs {
    const float* A[3]; int K[3];
    const float* B[3][3];
    const float* Breg; long breg_stride; const int* node_region;
    float* out[3];
    long M; int F, T, R;
};
int launch_model_dx(const ModelDxArgs& a, hipStream_t st);
// dx (nrows, F, T) = unpack(init + A^T P + L^T Q) over the transposed merged CSR (spmm_dual_t.hip); P, Q, init (nrows, T F) packed rows
int launch_spmm_dual_t(const int* rowptr, const int* col, const float* val_a, const float* val_l, const float* P, const float* Q,
                       const float* init, float* dx, int nrows, int F, int T, hipStream_t st);
int cell_bwd_blocks(int num_nodes, int nodes_per_block);
int launch_att_bwd(const float* dp_partial, int nblocks, const float* probs, float* datt, int T, hipStream_t st);
// zero-hidden cell: hidden[n, :] = sum_t probs[t] * (1 - Z[n*T+t, :]) * Ht[n*T+t, :]
int launch_blend0_fwd(const float* Z, const float* Ht, const float* probs, float* hidden, int num_nodes, int T, int C, hipStream_t st);
// GATConv attention aggregation on input rows (gat.hip)
int launch_gat_forward(const int* rowptr, const int* col, const float* x, const float* us, const float* ud, float slope, int N,
                       int T, int F, float* out, float* stats, hipStream_t st);
int launch_gat_backward(const int* rowptr, const int* col, const int* t_rowptr, const int* t_col, const float* x, const float* us,
                        float slope, int N, int T, int F, const float* dout, float* stats, float* dsd, hipStream_t st);
int launch_copy_f32(float* dst, const float* src, long n, hipStream_t st);
int launch_zero_f32(float* dst, long n, hipStream_t st);
int launch_mse_grad(const float* pred, const float* y, float* dpred, float* loss_out, long n, float scale, hipStream_t st);

// the regional embedding of the fp32 path at C = 256, F = 32 as a kernel of its own (embed.hip); region ids must ascend with the node number
bool embed_fp32_ok(long M, int C, int F, int T);
int launch_embed_fp32(const float* X, const float* LX, const float* A0, const float* Aall, const int* node_region, const float* bias,
                      float* out, long M, int T, int act, float slope, hipStream_t st);

// first ChebConv of SpatialGCN + ReLU + dropout mask + period sum (spatial.hip): S (N, 64); backward -> dW0, dW1 (64, F), db (64)
size_t spatial_slab_floats(int N, int T, int F);
int launch_spatial_fwd(const float* x, const float* lx, const float* w0, const float* w1, const float* b, const uint32_t* keep, int N,
                       int T, int F, float* S, hipStream_t st);
int launch_spatial_bwd(const float* x, const float* lx, const float* w0, const float* w1, const float* b, const uint32_t* keep,
                       const float* dS, int N, int T, int F, float* dw0, float* dw1, float* db, float* slab, hipStream_t st);

// STNorm (stnorm.hip): the whole model, one launch per layer plus the SNorm seams.  Parameter / gradient pointer tables: the
// ST_HEAD_PARAMS head entries (start_conv w, b, end_conv_1 w, b, end_conv_2 w, b), then ST_LAYER_PARAMS per layer (filter w, b,
// gate w, b, residual w, b, skip w, b, tn gamma, beta, sn gamma, beta; NULL where TNorm / SNorm is off).  run: 2 per layer.
struct StnDims { int num_nodes, batch, tnorm_group, seq_len, in_dim, out_dim, blocks, layers, tnorm, snorm, training; };
constexpr int ST_MAX_CH = 256, ST_HEAD_PARAMS = 6, ST_LAYER_PARAMS = 12;
bool stnorm_sizes(const StnDims& s, size_t* ws_floats, size_t* scratch_floats);
int launch_stnorm_fwd(const StnDims& s, const float* x, const float* const* P, float* const* run, float* out, float* ws, hipStream_t st);
int launch_stnorm_bwd(const StnDims& s, const float* x, const float* const* P, float* const* run, const float* dout, float* const* G,
                      const float* ws, float* scratch, hipStream_t st);

// STID (stid.hip): the whole per-node network in one forward launch; the backward is one launch plus a fixed-order reduction.
// Parameter / gradient pointer tables in state_dict order: node_emb (NULL when if_node is 0), time_series_emb_layer w, b, then per
// layer fc1 w, b, fc2 w, b, then regression_layer w, b: 3 + 4 * num_layer + 2 entries.
struct StidDims { int num_nodes, batch, input_len, in_features, input_dim, embed_dim, node_dim, num_layer, output_len, if_node; float dropout_p; };
constexpr int STID_MAX_LAYERS = 8, STID_MAX_KIN = 192, STID_MAX_OUT = 64, STID_MAX_WGS = 256;
bool stid_sizes(const StidDims& s, size_t* ws_floats, size_t* scratch_floats);
int launch_stid_fwd(const StidDims& s, const float* x, const float* const* P, const uint32_t* keep, float* out, float* ws, hipStream_t st);
int launch_stid_bwd(const StidDims& s, const float* x, const float* const* P, const uint32_t* keep, const float* dout, float* const* G,
                    const float* ws, float* scratch, hipStream_t st);

// One torch.nn.GRU layer over a whole sequence (gru.hip): a persistent forward and a persistent reverse pass, each workgroup owning
// GRU_RT batch rows for all steps, then fixed-order weight-gradient contractions.  x is read through three element strides.
struct GruDims { int seq_len, rows, input_size, hidden, training; long x_stride_seq, x_stride_row, x_stride_t; };
constexpr int GRU_HIDDEN = 256, GRU_RT = 8, GRU_MAX_INPUT = 255;
void gru_sizes(const GruDims& s, size_t* ws_floats, size_t* scratch_floats);
int launch_gru_fwd(const GruDims& s, const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                   const float* h0, float* out, float* h_last, float* ws, hipStream_t st);
int launch_relu_mask(const float* y, float* d, long n, hipStream_t st);      // d[i] = 0 where y[i] <= 0 (relu's gradient, in place)
// grads: dW_ih, dW_hh, db_ih, db_hh
int launch_gru_bwd(const GruDims& s, const float* x, const float* w_hh, const float* dout, const float* dh_last, float* const* grads,
                   float* dh0, const float* ws, float* scratch, hipStream_t st);

// STAEformer (staeformer.hip): the forward kernels between the dense layers; the inference launch sequence is stae_forward
// (api_baselines.hip), the trainable layer (nn.SelfAttentionLayer) composes the op-site entry points in functional.py.
// Parameter pointer table in state_dict order: node_emb, adaptive_embedding, input_proj w, b, tod_embedding, dow_embedding (NULL
// where the width is 0), output_proj w, b, then STAE_LAYER_PARAMS per layer, temporal layers first (attn.FC_Q w, b, FC_K, FC_V,
// out_proj, feed_forward.0 w, b, feed_forward.2 w, b, ln1 w, b, ln2 w, b).
struct StaeDims {
    int batch, in_steps, num_nodes, in_features, input_dim, e_in, e_tod, e_dow, e_sp, e_adp, steps_per_day, days_per_week, num_heads,
        ff_dim, num_layers, out_steps, output_dim;
    float ln_eps;
};
constexpr int STAE_HEAD_DIM = 32, STAE_MAX_DIM = 256, STAE_MAX_FF = 1024, STAE_MAX_LAYERS = 8, STAE_MAX_OUT = 64, STAE_HEAD_PARAMS = 8,
              STAE_LAYER_PARAMS = 16;
inline int stae_model_dim(const StaeDims& s) { return s.e_in + s.e_tod + s.e_dow + s.e_sp + s.e_adp; }
// lse (M, heads), optional: the training forward also stores each (row, head)'s log-sum-exp of the scaled scores; out is the same bits
int launch_stae_attention(const float* q, const float* k, const float* v, long ld, int B, int T, int N, int heads, int axis, float* out,
                          long ldo, hipStream_t st, float* lse = nullptr);
int launch_stae_add_layernorm(const float* residual, const float* y, const float* gamma, const float* beta, float eps, long M, int D,
                              float* out, hipStream_t st);
int launch_stae_embed(const StaeDims& s, const float* x, const float* const* P, float* out, hipStream_t st);
// STAEformer training (staeformer_bwd.hip): the backward kernels between the dense layers, two launches each.
// Attention: out / dout rows at ldo, dq / dk / dv rows at one common ldg (three windows of one buffer are fine), lse from the
// training forward; scratch: stae_attention_bwd_scratch_floats floats (delta per (row, head), written by the query pass).
size_t stae_attention_bwd_scratch_floats(long M, int heads);
int launch_stae_attention_bwd(const float* q, const float* k, const float* v, long ld, const float* out, const float* dout, long ldo,
                              const float* lse, int B, int T, int N, int heads, int axis, float* dq, float* dk, float* dv, long ldg,
                              float* scratch, hipStream_t st);
// Add+LayerNorm: dz (the gradient of residual and of y; no alias with an input), dgamma, dbeta; scratch: per-wave partial sums.
size_t stae_add_layernorm_bwd_scratch_floats(long M, int D);
// keep (M, D / 32 words: bit j of word w keeps column 32 w + j), optional: the branch y went through dropout, z = residual + keep y s;
// dz is then the gradient of residual only and dy = keep dz s (M x D, written in the same pass) that of y
int launch_stae_add_layernorm_bwd(const float* residual, const float* y, const float* gamma, const float* dout, float eps, long M, int D,
                                  float* dz, float* dgamma, float* dbeta, float* scratch, hipStream_t st, const uint32_t* keep = nullptr,
                                  float s = 1.0f, float* dy = nullptr);
int launch_stae_output_proj(const StaeDims& s, const float* x, const float* w, const float* bias, float* out, hipStream_t st);
// Column sums of (nparts, width) partial rows in 256 interleaved running sums combined pairwise, scattered by segment (slab_reduce.h)
struct SlabSegs;
int launch_stae_col_reduce(const float* partial, long nparts, long width, const SlabSegs& segs, hipStream_t st);
// STAEformer whole-model training (staeformer_train.hip): keep-bit dropout folded into add+LayerNorm, and the gradients of the
// embedding and of the output projection.  grads of the embedding: node_emb, adaptive_embedding, input_proj w, b, tod, dow (the first
// six table entries; NULL where the width is 0).  dout of the output projection is read through four element strides.
constexpr int STAE_EMBED_BWD_MAX_LDS = 15360;      // floats of one chunk's partial: input_proj w, b and the two tables
int launch_stae_drop_add_layernorm(const float* residual, const float* y, const uint32_t* keep, float s, const float* gamma, const float* beta,
                                   float eps, long M, int D, float* out, hipStream_t st);
long stae_embed_bwd_partial_floats(const StaeDims& s);
size_t stae_embed_bwd_scratch_floats(const StaeDims& s);
int launch_stae_embed_bwd(const StaeDims& s, const float* x, const float* dx0, float* const* grads, float* scratch, hipStream_t st);
size_t stae_output_proj_bwd_scratch_floats(const StaeDims& s);
int launch_stae_output_proj_bwd(const StaeDims& s, const float* x, const float* w, const float* dout, long sb, long so, long sn, long sc,
                                float* dx, float* dw, float* db, float* scratch, hipStream_t st);

// ---- per-device launch state ------------------------------------------------------------------------------------
// What a launcher needs to know about the device it is about to launch on is keyed by the device's ordinal, never by the process.
// A launcher that needs both helpers asks for the ordinal once and passes it on.
constexpr int MAX_DEVICES = 64;                 // ordinals the caches cover; past them every call asks the runtime
int current_device();                           // the ordinal current on the calling thread, -1 when no device answers
int device_cus(int dev = current_device());     // its CU count; 256 (an MI355X) when no device answers: sizes are computed on CPU-only hosts, too
int set_dynamic_lds(const void* kernel, int bytes);
// Raises the kernel's dynamic-LDS limit on the current device (= dev) the first time the instantiation is launched there.  Two
// threads racing on that first launch both raise it (harmless); the bit is only set once the limit stands.
template <auto Kernel>
int want_dynamic_lds(int bytes, int dev = current_device()) {
    static std::atomic<unsigned long long> done{0};
    const unsigned long long bit = (unsigned)dev < (unsigned)MAX_DEVICES ? 1ull << dev : 0;
    if (done.load(std::memory_order_acquire) & bit) return REGT_OK;
    if (int rc = set_dynamic_lds(reinterpret_cast<const void*>(Kernel), bytes)) return rc;
    done.fetch_or(bit, std::memory_order_release);
    return REGT_OK;
}
static_assert(MAX_DEVICES <= 64, "want_dynamic_lds keeps one bit per ordinal");

}  // namespace regt
