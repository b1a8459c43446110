// Recorder of tests/test_wgrad_choice_wave.py: when wgrad_pick (csrc/wgrad_dispatch.hip) chooses the wave-owned fp32 kernel, and what
// row chunks its chunker gives, without a GPU.  Built like tests/wgrad_plan/wgrad_plan.hip: the three weight-gradient units compiled
// host-only with tests/wgrad_plan/launch_log.h forced in (every hipLaunchKernelGGL becomes a report), the rest of the library stood
// in for below (256 CUs).  Pointers are fake, never dereferenced.  Lines:
//   pick <case>: <kernel's full name> grid=<blocks> lds=<dynamic bytes>      | pick <case>: rc=<code>
//   chunks <Nout> <M>: ok=<0|1> kchunk=<rows> nchunks=<n> pool=<floats make_layout (api_layout.hip) reserves for the slab
//                       regions of dUh and dUzr together at C = 256 and the smallest F, 4: max(layout's ~128 chunks, wgrad_chunk_bound(Nout,
//                       C + F, M)) x (Nout (C + F) + Nout) for Nout = C and 2C> min_rows=<wgrad_wave_min_rows>
#include <cxxabi.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "kernels.h"

namespace {

int g_mode = 0, g_wave = 1;
bool g_wide = false;
std::string g_launch;

float* fake(unsigned long long k) { return reinterpret_cast<float*>(0x100000000000ull + k * 0x4000000000ull); }      // 16-byte aligned

regt::WgradArgs args(int Nout, int Nin, long M) {
    regt::WgradArgs a{};
    a.P = fake(0); a.ldp = Nout; a.Nout = Nout;
    a.Q = fake(1); a.ldq = Nin; a.Nin = Nin;
    a.M = M;
    a.kchunk = 9376; a.nchunks = (int)((M + 9375) / 9376);          // the layout's ~128 chunks unless the chunker gives its own
    regt::wgrad_wide_chunking(Nout, Nin, M, &a.kchunk, &a.nchunks);
    a.slab = fake(2);
    a.colsum = 1;
    return a;
}
void pick(const char* name, const regt::WgradArgs& a) {
    g_launch.clear();
    const int rc = regt::launch_wgrad(a, nullptr);
    if (rc != 0) printf("pick %s: rc=%d\n", name, rc);
    else printf("pick %s: %s\n", name, g_launch.c_str());
}
void chunks(int Nout, long M) {
    int kc = -1, nc = -1;
    const bool ok = regt::wgrad_wave_shape(Nout, 256) && regt::wgrad_wave_chunking(Nout, M, &kc, &nc);
    const long C = 256, F = 4, lkc = ((M + 127) / 128 + 31) / 32 * 32, layout = (M + lkc - 1) / lkc;      // make_layout's L.nchunks
    long pool = 0;
    for (long no : {C, 2 * C}) {
        const long b = regt::wgrad_chunk_bound((int)no, (int)(C + F), M);
        pool += (b > layout ? b : layout) * (no * (C + F) + no);
    }
    printf("chunks %d %ld: ok=%d kchunk=%d nchunks=%d pool=%ld min_rows=%ld\n", Nout, M, ok ? 1 : 0, kc, nc, pool, regt::wgrad_wave_min_rows());
}

}  // namespace

extern "C" hipError_t hipGetLastError() { return hipSuccess; }

namespace wgrad_plan {
int all_csum_of(const regt::WgradArgs& a) { return a.all_csum; }
void log_launch(const std::type_info& tag, dim3 grid, dim3, size_t lds_bytes, int) {
    int status = 0;
    char* dem = abi::__cxa_demangle(tag.name(), nullptr, nullptr, &status);
    std::string name = dem ? dem : tag.name();
    free(dem);
    char buf[64];
    snprintf(buf, sizeof buf, " grid=%u lds=%zu", grid.x, lds_bytes);
    g_launch = name + buf;
}
}  // namespace wgrad_plan

namespace regt {
void set_error(const char*, ...) {}
int option(OptId id) {
    switch (id) {
        case OPT_WGRAD_RING: return 6;
        case OPT_WGRAD_TILE: return 256;
        case OPT_WGRAD_RING256: return 2;
        case OPT_WGRAD_BNW64: return 1;
        case OPT_WGRAD_WAVE: return g_wave;
        default: return 0;
    }
}
int gemm_mode() { return g_mode; }
bool fp32_core_wide() { return g_wide; }
int current_device() { return -1; }
int device_cus(int) { return 256; }
int set_dynamic_lds(const void*, int) { return REGT_OK; }
}  // namespace regt

int main() {
    const long M3 = 1200000, MIN = regt::wgrad_wave_min_rows();
    // chosen: the two wide gradients of the cell at cfg-3 and at the smallest accepted M
    pick("dUh_cfg3", args(256, 256, M3));
    pick("dUzr_cfg3", args(512, 256, M3));
    pick("dUh_min", args(256, 256, MIN));
    pick("dUzr_min", args(512, 256, MIN));
    { regt::WgradArgs a = args(512, 256, M3); a.ldp = 1024; a.P = fake(0) + 512; pick("dUzr_window", a); }
    // not chosen
    pick("small_m", args(256, 256, MIN - 1));
    pick("tpims_m", args(256, 256, 36000));
    pick("f_wide_rhs", args(256, 32, M3));
    pick("f64_rhs", args(256, 64, M3));
    pick("nin128", args(256, 128, M3));
    pick("nout384", args(384, 256, M3));
    { regt::WgradArgs a = args(256, 256, M3); a.P = fake(0) + 1; pick("misaligned_p", a); }
    { regt::WgradArgs a = args(256, 256, M3); a.Q = fake(1) + 2; pick("misaligned_q", a); }
    { regt::WgradArgs a = args(256, 256, M3); a.kchunk = 9376; a.nchunks = 128; pick("layout_chunks", a); }
    g_wave = 0; pick("option_off", args(256, 256, M3)); pick("option_off_dUzr", args(512, 256, M3)); g_wave = 1;
    g_wide = true; pick("wide_core", args(256, 256, M3)); g_wide = false;
    g_mode = 1; pick("bf16x3", args(256, 256, M3)); g_mode = 0;
    g_mode = 2;
    { regt::WgradArgs a = args(256, 256, M3); a.p_bf16 = a.q_bf16 = 1; pick("bf16_operands", a); }
    g_mode = 0;
    for (int Nout : {256, 512})
        for (long M : {M3, MIN, MIN - 1, MIN + 1, 3L * MIN + 12345, 40000000L}) chunks(Nout, M);
    return 0;
}
