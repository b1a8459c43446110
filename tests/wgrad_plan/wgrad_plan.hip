// Launch-plan recorder of the weight gradients (tests/test_wgrad_plan_cpu.py): which kernel launch_wgrad picks for given arguments and
// switches, with which grid and dynamic LDS, pinned without a GPU.  Links the weight-gradient units compiled host-only with
// launch_log.h forced in, which turns every hipLaunchKernelGGL into a report, and stands in for what they ask of the rest of the
// library: option, gemm_mode, fp32_core_wide, device_cus (256), current_device (-1: no ordinal, so want_dynamic_lds never
// remembers a request and every one reaches set_dynamic_lds below), set_dynamic_lds, set_error.  Pointers are fake, never dereferenced.
// One line per case:
//   <case>: <kernel's full name> grid=<blocks> block=<threads> lds=<dynamic bytes> lds_limit=<bytes asked of set_dynamic_lds | -> all_csum=<0|1>
//   <case>: rc=<code> error: <text>
//
// tests/golden/wgrad_plan.txt was recorded from csrc/wgrad.hip as it was BEFORE it was cut into wgrad_dispatch.hip, wgrad_fp32.hip,
// wgrad_bf16.hip and wgrad_reduce.hip (commit 39d0a81), its text untouched, with this same source and shim:
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 -O1 -I regt-gcn_amd/csrc -include tests/wgrad_plan/launch_log.h \
//         tests/wgrad_plan/wgrad_plan.hip <that commit's>/regt-gcn_amd/csrc/wgrad.hip -Wl,--unresolved-symbols=ignore-all \
//         -o wgrad_plan && ./wgrad_plan
// (a host-only compile of a unit with kernels still refers to the unit's device image; the reference stays open, nothing launches).
// The committed test builds the same line with the three current units in place of wgrad.hip and compares.
#include <cxxabi.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "kernels.h"

namespace {

struct Case {
    std::string name;
    int mode = 0;                   // gemm_mode(): 0 fp32, 1 bf16x3, 2 bf16
    bool wide = false;              // fp32_core_wide()
    int ring = 6, tile = 256, ring256 = 2, bnw64 = 1;
    regt::WgradArgs a;
};
Case g_case;
std::string g_launch, g_error;
long g_lds_limit = -1;
std::set<std::string> g_kernels;

float* fake(unsigned long long k) { return reinterpret_cast<float*>(0x100000000000ull + k * 0x4000000000ull); }      // 16-byte aligned

Case base(const std::string& name, int mode, int Nout, int Nin) {
    Case c;
    c.name = name;
    c.mode = mode;
    regt::WgradArgs& a = c.a;
    a.P = fake(0); a.ldp = Nout; a.Nout = Nout;
    a.Q = fake(1); a.ldq = Nin; a.Nin = Nin;
    a.q_relu = 0;
    a.M = 4096; a.kchunk = 1024; a.chunk_tab = nullptr; a.nchunks = 4;
    a.slab = fake(2);
    a.colsum = 1;
    return c;
}
Case with_q2(Case c, int nin_split) {
    c.a.Q2 = fake(3);
    c.a.nin_split = nin_split;
    c.a.ldq = nin_split;
    c.a.ldq2 = c.a.Nin - nin_split;
    return c;
}
Case bf16(Case c, int p, int q) { c.a.p_bf16 = p; c.a.q_bf16 = q; return c; }

void run(const Case& c) {
    g_case = c;
    g_launch.clear();
    g_error.clear();
    g_lds_limit = -1;
    const int rc = regt::launch_wgrad(c.a, nullptr);
    if (rc != 0 || !g_error.empty()) printf("%s: rc=%d error: %s\n", c.name.c_str(), rc, g_error.c_str());
    else printf("%s: %s\n", c.name.c_str(), g_launch.empty() ? "(no launch)" : g_launch.c_str());
}

void all_cases() {
    const char* mode_name[3] = {"fp32", "bf16x3", "bf16"};
    // the arithmetics, with and without the wide fp32 core: Nin <= 32, 33-64 with wgrad_bnw64 on and off, > 64, rows that are no multiple of 4
    for (int mode = 0; mode < 3; ++mode)
        for (int wide = 0; wide < 2; ++wide) {
            const std::string pre = std::string(mode_name[mode]) + (wide ? "_widecore" : "");
            auto arith = [&](const char* what, int Nout, int Nin) { Case c = base(pre + "_" + what, mode, Nout, Nin); c.wide = wide; return c; };
            run(arith("nin32", 256, 32));
            run(arith("nin64_bnw64", 256, 64));
            { Case c = arith("nin64_bnw32", 256, 64); c.bnw64 = 0; run(c); }
            run(arith("nin128", 256, 128));
            run(arith("nin160", 256, 160));
            { Case c = arith("generic_nin32", 256, 32); c.a.ldp = 258; run(c); }
            { Case c = arith("generic_nin128", 256, 128); c.a.ldp = 258; run(c); }
        }
    // operands stored as bf16
    run(bf16(base("fp32_pbf_nin32", 0, 256, 32), 1, 0));
    run(bf16(base("bf16_pbf_nin32", 2, 256, 32), 1, 0));
    run(bf16(base("bf16_qbf_nin32", 2, 256, 32), 0, 1));
    for (int p = 0; p < 2; ++p)
        for (int q = 0; q < 2; ++q) {
            Case c = bf16(base("bf16_p" + std::to_string(p) + "_q" + std::to_string(q) + "_ring0", 2, 384, 128), p, q);
            c.ring = 0;
            run(c);
            c.name = "bf16_p" + std::to_string(p) + "_q" + std::to_string(q) + "_ring6";
            c.ring = 6;
            run(c);
        }
    // two-part right-hand side
    run(with_q2(base("fp32_q2_inside_tile64", 0, 256, 64), 32));
    { Case c = with_q2(base("fp32_q2_inside_tile64_bnw32", 0, 256, 64), 32); c.bnw64 = 0; run(c); }
    run(with_q2(base("fp32_q2_nin128", 0, 256, 128), 64));
    run(with_q2(base("bf16x3_q2_nin128", 1, 256, 128), 64));
    run(with_q2(base("bf16_q2_nin128_split64", 2, 256, 128), 64));
    run(with_q2(base("bf16_q2_nin160", 2, 256, 160), 32));
    { Case c = with_q2(base("bf16_q2_widecore", 2, 256, 128), 64); c.wide = true; run(c); }
    run(bf16(with_q2(base("bf16_q2_stored_on_128", 2, 384, 256), 128), 1, 1));
    run(bf16(with_q2(base("bf16_q2_stored_off_128", 2, 384, 128), 64), 1, 1));
    run(bf16(with_q2(base("bf16_q2_stored_nin320_on_128", 2, 384, 320), 256), 1, 1));
    { Case c = with_q2(base("fp32_q2_relu", 0, 256, 64), 32); c.a.q_relu = 1; run(c); }
    { Case c = with_q2(base("bf16_q2_relu", 2, 256, 128), 64); c.a.q_relu = 1; run(c); }
    { Case c = base("fp32_relu_nin128", 0, 256, 128); c.a.q_relu = 1; run(c); }
    // ring and tile switches (both operands stored as bf16)
    for (int ring : {0, 4, 6, 8}) {
        Case c = bf16(base("ring" + std::to_string(ring) + "_tile128", 2, 256, 128), 1, 1);
        c.ring = ring; c.tile = 128;
        run(c);
    }
    for (int tile : {128, 256})
        for (int Nout : {256, 384})
            for (int r256 : {2, 4}) {
                Case c = bf16(base("tile" + std::to_string(tile) + "_nout" + std::to_string(Nout) + "_ring256_" + std::to_string(r256), 2, Nout, 128), 1, 1);
                c.tile = tile; c.ring256 = r256;
                run(c);
            }
    { Case c = bf16(base("ring0_tile256", 2, 256, 128), 1, 1); c.ring = 0; run(c); }
    { Case c = bf16(base("ring8_tile256_nout384", 2, 384, 128), 1, 1); c.ring = 8; run(c); }
    // the ring's size bound: chunk rows x row bytes reach 2^31 (rows_max = kchunk + 32 = 32768, 2 bytes x 32768 elements per row) and just do not
    { Case c = bf16(base("ring_bound_reached", 2, 256, 128), 1, 1); c.a.ldp = 32768; c.a.kchunk = 32736; c.a.M = 4 * 32736; run(c); }
    { Case c = bf16(base("ring_bound_below", 2, 256, 128), 1, 1); c.a.ldp = 32768; c.a.kchunk = 32704; c.a.M = 4 * 32704; run(c); }
    { Case c = bf16(base("ring_bound_chunk_tab", 2, 256, 128), 1, 1); c.a.chunk_tab = reinterpret_cast<const int*>(fake(4)); c.a.ldp = 32768; c.a.M = 32768; run(c); }
    { Case c = bf16(base("ring_chunk_tab", 2, 256, 128), 1, 1); c.a.chunk_tab = reinterpret_cast<const int*>(fake(4)); c.a.kchunk = 1 << 20; run(c); }
    { Case c = base("fp32_kchunk_past_65536", 0, 256, 128); c.a.kchunk = 65568; c.a.M = 4 * 65568; run(c); }
    { Case c = base("fp32_no_colsum_tail_tiles", 0, 132, 36); c.a.colsum = 0; c.a.nchunks = 11; run(c); }
    // one case per refusal, in the order of the checks
    run(base("refuse_empty", 0, 0, 32));
    { Case c = base("refuse_blocks", 0, 1 << 20, 32); c.a.nchunks = 1 << 18; run(c); }
    run(with_q2(base("refuse_q2_not_tileable", 0, 256, 64), 16));
    { Case c = bf16(base("refuse_bf16_not_tileable", 0, 256, 32), 1, 0); c.a.ldp = 258; run(c); }
    { Case c = bf16(base("refuse_bf16_rows_of_8", 2, 132, 128), 1, 0); c.a.ldp = 136; run(c); }
    run(bf16(base("refuse_bf16_on_fp32", 0, 256, 128), 1, 0));
    { Case c = bf16(base("refuse_bf16_on_fp32_wide", 0, 256, 128), 0, 1); c.wide = true; run(c); }
    run(bf16(base("refuse_skinny_qbf", 0, 256, 32), 0, 1));
    { Case c = bf16(base("refuse_skinny_pbf_rows_of_8", 0, 132, 32), 1, 0); c.a.ldp = 132; run(c); }
}

}  // namespace

extern "C" hipError_t hipGetLastError() { return hipSuccess; }

namespace wgrad_plan {
int all_csum_of(const regt::WgradArgs& a) { return a.all_csum; }
void log_launch(const std::type_info& tag, dim3 grid, dim3 block, size_t lds_bytes, int all_csum) {
    // "wgrad_plan::KernelTag<&(void regt::wgrad_kernel<128, false>(regt::WgradArgs))>"
    int status = 0;
    char* dem = abi::__cxa_demangle(tag.name(), nullptr, nullptr, &status);
    std::string name = dem ? dem : tag.name();
    free(dem);
    const size_t open = name.find("<&");                        // (a kernel that is no template: "wgrad_plan::KernelTag<&regt::wgrad3_kernel>")
    if (open != std::string::npos && name[open + 2] == '(') name = name.substr(open + 3, name.size() - open - 5);
    else if (open != std::string::npos) name = name.substr(open + 2, name.size() - open - 3);
    g_kernels.insert(name);
    char buf[256];
    snprintf(buf, sizeof buf, " grid=%u,%u,%u block=%u lds=%zu lds_limit=%s all_csum=%d", grid.x, grid.y, grid.z, block.x, lds_bytes,
             g_lds_limit < 0 ? "-" : std::to_string(g_lds_limit).c_str(), all_csum);
    if (!g_launch.empty()) g_launch += " | ";
    g_launch += name + buf;
}
}  // namespace wgrad_plan

namespace regt {

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}
int option(OptId id) {
    switch (id) {
        case OPT_WGRAD_RING: return g_case.ring;
        case OPT_WGRAD_TILE: return g_case.tile;
        case OPT_WGRAD_RING256: return g_case.ring256;
        case OPT_WGRAD_BNW64: return g_case.bnw64;
        case OPT_WGRAD_WAVE: return 1;
        default: return 0;
    }
}
int gemm_mode() { return g_case.mode; }
bool fp32_core_wide() { return g_case.wide; }
int current_device() { return -1; }
int device_cus(int) { return 256; }
int set_dynamic_lds(const void*, int bytes) { g_lds_limit = bytes; return REGT_OK; }

}  // namespace regt

int main() {
    all_cases();
    printf("kernels");
    for (const std::string& k : g_kernels) printf(" %s;", k.c_str());
    printf("\n");
    return 0;
}
