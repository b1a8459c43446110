// Launch-plan recorder of the neighbour aggregation and of the snapshot pack / convert launchers (tests/test_spmm_plan_cpu.py): which
// kernel launch_pack_x, launch_pack_x_bf16, launch_cvt_rows_bf16, launch_spmm_csr, launch_spmm_dual(_x) and launch_spmm_dual_bf16
// pick for given arguments and switches, with which grid, dynamic LDS and arguments, pinned without a GPU.  Links the units compiled
// host-only with launch_log.h forced in, which turns every hipLaunchKernelGGL into a report, and stands in for what they ask of the
// rest of the library: option (spmm_pl, spmm_rows from the case), set_error.  Pointers are fake, never dereferenced.
// One line per case:
//   <case>: <kernel's full name> grid=<x,y,z> block=<threads> lds=<dynamic bytes> args=<every launch argument in order> [| next launch]
//   <case>: rc=<code> error: <text>
// Pointer arguments print as <buffer>+<byte offset>: rowptr, col, val (val_a), val_l, X, Y (YA), YL, or null.
//   spmm_plan               the built-in cases, then the list of kernels reached
//   spmm_plan --cases FILE  one case per line of FILE: <name> csr <nrows> <nrows_x> <W> <nstack> <spmm_rows> <spmm_pl>
//                                                      <name> dual|bf16 <nnodes> <x_rows> <W> <spmm_rows> <spmm_pl>
//
// tests/golden/spmm_plan.txt was recorded from csrc/spmm.hip as it was BEFORE it was cut into pack.hip, spmm_dispatch.hip,
// spmm_csr.hip and spmm_panel.hip (commit 2f958e5), its text untouched, with this same source and shim:
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 -O1 -I regt-gcn_amd/csrc -include tests/spmm_plan/launch_log.h \
//         tests/spmm_plan/spmm_plan.hip <that commit's>/regt-gcn_amd/csrc/spmm.hip -Wl,--unresolved-symbols=ignore-all \
//         -o spmm_plan && ./spmm_plan
// (a host-only compile of a unit with kernels still refers to the unit's device image; the reference stays open, nothing launches).
// The committed test builds the same line with the current units in place of spmm.hip and compares.
#include <cxxabi.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>
#include <string>

#include "kernels.h"

namespace {

int g_rows = 0, g_pl = 0;           // option(OPT_SPMM_ROWS), option(OPT_SPMM_PL)
std::string g_launch, g_error;
std::set<std::string> g_kernels;

constexpr unsigned long long ARENA0 = 0x100000000000ull, ARENA_STEP = 0x4000000000ull;      // 256 GB apart, 16-byte aligned
const char* const BUFS[] = {"rowptr", "col", "val", "val_l", "X", "Y", "YL"};
template <class T = float> T* fake(int k, long off = 0) { return reinterpret_cast<T*>(ARENA0 + k * ARENA_STEP + off); }
const int* RP = fake<const int>(0);
const int* COL = fake<const int>(1);
const float* VA = fake<const float>(2);
const float* VL = fake<const float>(3);

void begin(int rows, int pl) {
    g_rows = rows;
    g_pl = pl;
    g_launch.clear();
    g_error.clear();
}
void end(const std::string& name, int rc) {
    if (rc != 0 || !g_error.empty()) printf("%s: rc=%d error: %s\n", name.c_str(), rc, g_error.c_str());
    else printf("%s: %s\n", name.c_str(), g_launch.empty() ? "(no launch)" : g_launch.c_str());
}

void pack(const std::string& name, int N, int F, int T, long xoff = 0, long poff = 0) {
    begin(0, 0);
    end(name, regt::launch_pack_x(fake(4, xoff), fake(5, poff), N, F, T, nullptr));
}
void pack_bf(const std::string& name, int N, int F, int T, long xoff = 0, long poff = 0) {
    begin(0, 0);
    end(name, regt::launch_pack_x_bf16(fake(4, xoff), fake<void>(5, poff), N, F, T, nullptr));
}
void cvt(const std::string& name, long n) {
    begin(0, 0);
    end(name, regt::launch_cvt_rows_bf16(fake(4), fake<void>(5), n, nullptr));
}
void csr(const std::string& name, int nrows, int nrows_x, int W, int nstack, int rows = 0, int pl = 0, long xoff = 0, long yoff = 0) {
    begin(rows, pl);
    end(name, regt::launch_spmm_csr(RP, COL, VA, fake(4, xoff), fake(5, yoff), nrows, nrows_x, W, nstack, nullptr));
}
void dual(const std::string& name, int nnodes, int x_rows, int W, int rows = 0, int pl = 0) {
    begin(rows, pl);
    end(name, regt::launch_spmm_dual_x(RP, COL, VA, VL, fake(4), fake(5), fake(6), nnodes, x_rows, W, nullptr));
}
void dual_bf(const std::string& name, int nnodes, int x_rows, int W, int rows = 0, int pl = 0) {
    begin(rows, pl);
    end(name, regt::launch_spmm_dual_bf16(RP, COL, VA, VL, fake<void>(4), fake<void>(5), fake<void>(6), nnodes, x_rows, W, nullptr));
}

std::string num(long v) { return std::to_string(v); }

constexpr int WIDE_N = 147456;          // cdiv(n, 8) * 256 == SP_WIDE_SLICE_MAX: the last node count with 256-byte panels
constexpr int BIG_N = 41003;            // tests/op_bars.py LARGE_N
constexpr int ROWS_N = 60003;           // 128-float rows of X pass 24 MB; no multiple of 8

void all_cases() {
    // ---- pack / convert ----
    pack("pack_lds", 1000, 32, 12);
    pack("pack_f_not_4", 1000, 30, 12);
    pack("pack_ft_4096", 1000, 256, 16);
    pack("pack_ft_4100", 1000, 4, 1025);
    pack("pack_x_misaligned", 1000, 32, 12, 4, 0);
    pack("pack_xp_misaligned", 1000, 32, 12, 0, 8);
    pack("pack_lds_blocks_4096", 40960, 32, 12);
    pack("pack_lds_blocks_capped", 40970, 32, 12);
    pack("pack_blocks_8192", 8192 * 256, 1, 1);
    pack("pack_blocks_capped", 8192 * 256 + 1, 1, 1);
    pack_bf("packbf_lds", 1000, 32, 12);
    pack_bf("packbf_refuse_f_not_8", 1000, 12, 12);
    pack_bf("packbf_ft_4096", 1000, 256, 16);
    pack_bf("packbf_ft_4104", 1000, 8, 513);
    pack_bf("packbf_x_misaligned", 1000, 32, 12, 4, 0);
    pack_bf("packbf_xp_misaligned", 1000, 32, 12, 0, 8);
    pack_bf("packbf_lds_blocks_4096", 40960, 32, 12);
    pack_bf("packbf_lds_blocks_capped", 40970, 32, 12);
    pack_bf("packbf_blocks_16384", 16384 * 256, 8, 1, 0, 8);
    pack_bf("packbf_blocks_capped", 16384 * 256 + 1, 8, 1, 0, 8);
    cvt("cvt", 8000);
    cvt("cvt_refuse_n_not_8", 8004);
    cvt("cvt_blocks_16384", 8L * 256 * 16384);
    cvt("cvt_blocks_capped", 8L * 256 * 16384 + 8);

    // ---- launch_spmm_csr ----
    // the width ladder: every rung at its upper edge and one float4 past it; column passes (513: a one-float4 last pass)
    for (int W4 : {1, 8, 9, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 192, 193, 256, 257, 512, 513, 1024, 1100})
        csr("csr_w4_" + num(W4), 600, 600, 4 * W4, 1);
    csr("csr_blocks_16384", 16384 * 32, 600, 16, 1);
    csr("csr_blocks_capped", 16384 * 32 + 1, 600, 16, 1);
    csr("csr_wide_rows_large_x", BIG_N, BIG_N, 4 * 520, 1);       // W4 % 8 == 0, X > 24 MB, W4 > 512: the panel gate comes first
    // the panel gate, each side of each condition
    csr("csr_gate_w4_36", BIG_N, BIG_N, 144, 1);
    csr("csr_gate_w4_40", BIG_N, BIG_N, 160, 1);
    csr("csr_gate_x_24mb", 49152, 49152, 128, 1);
    csr("csr_gate_x_24mb_one_row_more", 49152, 49153, 128, 1);
    csr("csr_gate_nodes_4095", 4095, 49153, 128, 1);
    csr("csr_gate_nodes_4096", 4096, 49153, 128, 1);
    csr("csr_gate_nstack2_nodes_4095", 8190, 49153, 128, 2);
    csr("csr_gate_nstack2_nodes_4096", 8192, 49153, 128, 2);
    // panel width: W4 % 16, the slice bound, spmm_pl
    for (int n : {WIDE_N, WIDE_N + 1})
        for (int W4 : {32, 40})
            for (int pl : {0, 8, 16})
                for (int nstack : {1, 2})
                    csr("csr_panel_n" + num(n) + "_w4_" + num(W4) + "_pl" + num(pl) + "_nstack" + num(nstack), n * nstack, n, 4 * W4, nstack, 0, pl);
    // the row-block kernel: wanted or not, one operator only, each clause of rows_ok (whole panels cannot fail behind the W4 % 8 gate)
    for (int W4 : {32, 40})
        for (int rows : {0, 1})
            for (int pl : {0, 8, 16})
                csr("csr_rows" + num(rows) + "_w4_" + num(W4) + "_pl" + num(pl), ROWS_N, ROWS_N, 4 * W4, 1, rows, pl);
    csr("csr_rows1_nstack2", 2 * ROWS_N, ROWS_N, 128, 2, 1);
    csr("csr_rows1_x_bytes_below", BIG_N, 8388599, 128, 1, 1);
    csr("csr_rows1_x_bytes_at", BIG_N, 8388600, 128, 1, 1);
    csr("csr_rows1_y_bytes_below", 486295, 4096, 2208, 1, 1);
    csr("csr_rows1_y_bytes_at", 486296, 4096, 2208, 1, 1);
    csr("csr_rows1_rpg_8", 491520, 491520, 128, 1, 1);
    csr("csr_rows1_rpg_9", 491521, 491521, 128, 1, 1);
    // refusals
    csr("csr_refuse_empty", 0, 600, 128, 1);
    csr("csr_refuse_no_width", 600, 600, 0, 1);
    csr("csr_refuse_w_not_4", 600, 600, 30, 1);
    csr("csr_refuse_x_misaligned", 600, 600, 128, 1, 0, 0, 4, 0);
    csr("csr_refuse_y_misaligned", 600, 600, 128, 1, 0, 0, 0, 8);
    csr("csr_refuse_nstack_0", 600, 600, 128, 0);
    csr("csr_refuse_nstack_odd", 601, 600, 128, 2);
    csr("csr_grid_below", 8388608, 8388608, 4 * 65528, 1);
    csr("csr_refuse_grid", 8388608, 8388608, 4 * 65536, 1);
    csr("csr_refuse_grid_nstack2", 8388608, 4194304, 4 * 65536, 2);

    // ---- launch_spmm_dual_x ----
    dual("dual_refuse_w_not_4", 600, 600, 30);
    dual("dual_refuse_empty", 0, 600, 128);
    for (int W4 : {1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512})
        dual("dual_w4_" + num(W4), 600, 600, 4 * W4);
    dual("dual_refuse_w4_513", 600, 600, 4 * 513);
    dual("dual_small_x_w4_520", 600, 600, 4 * 520);                 // whole panels, X <= 24 MB but W4 > 512: panel kernel
    dual("dual_large_x_w4_36", BIG_N, BIG_N, 144);                  // not whole panels: lane groups whatever the size
    dual("dual_gate_x_24mb", 49152, 49152, 128);
    dual("dual_gate_x_24mb_one_row_more", 49153, 49153, 128);
    dual("dual_gate_halo_rows_count", 49152, 49153, 128);           // x_rows, not nnodes, is what the gate measures
    dual("dual_blocks_16384", 16384 * 32, 16384 * 32, 28);
    dual("dual_blocks_capped", 16384 * 32 + 1, 16384 * 32 + 1, 28);
    for (int n : {WIDE_N, WIDE_N + 1})
        for (int W4 : {32, 40})
            for (int pl : {0, 8, 16})
                dual("dual_panel_n" + num(n) + "_w4_" + num(W4) + "_pl" + num(pl), n, n, 4 * W4, 0, pl);
    for (int W4 : {32, 40})
        for (int rows : {0, 1})
            for (int pl : {0, 8, 16})
                dual("dual_rows" + num(rows) + "_w4_" + num(W4) + "_pl" + num(pl), ROWS_N, ROWS_N, 4 * W4, rows, pl);
    for (int rows : {0, 1}) dual("dual_halo_rows" + num(rows), BIG_N, 50000, 128, rows);
    dual("dual_rows1_x_bytes_below", BIG_N, 8388599, 128, 1);
    dual("dual_rows1_x_bytes_at", BIG_N, 8388600, 128, 1);
    dual("dual_rows1_y_bytes_below", 486295, 4096, 2208, 1);
    dual("dual_rows1_y_bytes_at", 486296, 4096, 2208, 1);
    dual("dual_rows1_rpg_8", 491520, 491520, 128, 1);
    dual("dual_rows1_rpg_9", 491521, 491521, 128, 1);
    dual("dual_grid_below", 8388608, 8388608, 4 * 65528);
    dual("dual_refuse_grid", 8388608, 8388608, 4 * 65536);
    // launch_spmm_dual: x_rows = nnodes
    begin(0, 0);
    end("dual_plain_entry", regt::launch_spmm_dual(RP, COL, VA, VL, fake(4), fake(5), fake(6), BIG_N, 192, nullptr));

    // ---- launch_spmm_dual_bf16 ----
    dual_bf("bf16_refuse_w_not_64", BIG_N, BIG_N, 96);
    dual_bf("bf16_refuse_empty", 0, BIG_N, 128);
    dual_bf("bf16_x_bytes_below", BIG_N, 16777199, 128);
    dual_bf("bf16_refuse_x_4gb", BIG_N, 16777200, 128);
    dual_bf("bf16_refuse_x_4gb_rows1", BIG_N, 16777200, 128, 1);
    for (int n : {600, WIDE_N, WIDE_N + 1})
        for (int W : {128, 192})
            for (int pl : {0, 8, 16})
                dual_bf("bf16_panel_n" + num(n) + "_w" + num(W) + "_pl" + num(pl), n, n, W, 0, pl);
    for (int W : {128, 192})
        for (int rows : {0, 1})
            for (int pl : {0, 8, 16})
                dual_bf("bf16_rows" + num(rows) + "_w" + num(W) + "_pl" + num(pl), BIG_N, BIG_N, W, rows, pl);
    dual_bf("bf16_halo_rows1", BIG_N, 50000, 128, 1);
    dual_bf("bf16_rows1_rpg_8", 307200, 307200, 192, 1);
    dual_bf("bf16_rows1_rpg_9", 307201, 307201, 192, 1);
    // the fp32 forms refuse the row-block kernel when nnodes * rowbytes does not fit 32 bits (rows_ok); this form does not ask
    dual_bf("bf16_rows1_y_bytes_past_4gb", 307200, 4096, 7040, 1);
    dual_bf("bf16_rows0_y_bytes_past_4gb", 307200, 4096, 7040, 0);
    dual_bf("bf16_grid_below", 8388608, 4000, 8 * 65528);
    dual_bf("bf16_refuse_grid", 8388608, 4000, 8 * 65536);
}

int file_cases(const char* path) {
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "spmm_plan: cannot read %s\n", path); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string name, op;
        long v[6] = {0, 0, 0, 0, 0, 0};
        if (!(s >> name >> op)) continue;
        const int want = op == "csr" ? 6 : 5;
        for (int i = 0; i < want; ++i)
            if (!(s >> v[i])) { fprintf(stderr, "spmm_plan: short line: %s\n", line.c_str()); return 2; }
        if (op == "csr") csr(name, (int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5]);
        else if (op == "dual") dual(name, (int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4]);
        else if (op == "bf16") dual_bf(name, (int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4]);
        else { fprintf(stderr, "spmm_plan: unknown op %s\n", op.c_str()); return 2; }
    }
    return 0;
}

}  // namespace

extern "C" hipError_t hipGetLastError() { return hipSuccess; }

namespace spmm_plan {
std::string ptr_text(const void* p) {
    if (!p) return "null";
    const unsigned long long a = reinterpret_cast<unsigned long long>(p);
    if (a < ARENA0 || (a - ARENA0) / ARENA_STEP >= sizeof BUFS / sizeof *BUFS) return "stray";
    return std::string(BUFS[(a - ARENA0) / ARENA_STEP]) + "+" + std::to_string((a - ARENA0) % ARENA_STEP);
}
void log_launch(const std::type_info& tag, dim3 grid, dim3 block, size_t lds_bytes, const std::string& args) {
    // "spmm_plan::KernelTag<&(void regt::spmm_panel_kernel<8>(int const*, ...))>"; a kernel that is no template: "...<&regt::pack_x_kernel>"
    int status = 0;
    char* dem = abi::__cxa_demangle(tag.name(), nullptr, nullptr, &status);
    std::string name = dem ? dem : tag.name();
    free(dem);
    const size_t open = name.find("<&");
    if (open != std::string::npos && name[open + 2] == '(') name = name.substr(open + 3, name.size() - open - 5);
    else if (open != std::string::npos) name = name.substr(open + 2, name.size() - open - 3);
    g_kernels.insert(name);
    char buf[160];
    snprintf(buf, sizeof buf, " grid=%u,%u,%u block=%u lds=%zu args=", grid.x, grid.y, grid.z, block.x, lds_bytes);
    if (!g_launch.empty()) g_launch += " | ";
    g_launch += name + buf + args;
}
}  // namespace spmm_plan

namespace regt {

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}
int option(OptId id) { return id == OPT_SPMM_ROWS ? g_rows : id == OPT_SPMM_PL ? g_pl : 0; }

}  // namespace regt

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "--cases")) return file_cases(argv[2]);
    all_cases();
    printf("kernels");
    for (const std::string& k : g_kernels) printf(" %s;", k.c_str());
    printf("\n");
    return 0;
}
