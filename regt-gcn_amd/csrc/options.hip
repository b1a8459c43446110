// The table of runtime switches (options.h) and the only getenv of the library.
#include <limits.h>
#include <stdlib.h>

#include <atomic>

#include "common.h"
#include "options.h"

namespace regt {
namespace {

// how a variable's text becomes a value: atoi | 1 where it equals the row's word, else 0 | the words of REGT_GEMM_MODE
enum Parse { P_INT, P_WORD, P_MODE };
// how a value is normalised before it is stored (regt_set_option, and what the environment gave)
enum Clamp { C_NONE, C_BOOL, C_ROWS, C_NONNEG, C_TILE, C_RING256, C_PAIRS, C_MODE };

struct Row { OptId id; const char* name; const char* env; int dflt; Parse parse; const char* word; Clamp clamp; };

// One row per switch, one row per line, in the order of OptId (tests/test_abi_cpu.py reads the names from here).
// name = nullptr: environment-only; env = nullptr: regt_set_option only.
constexpr Row ROWS[] = {
    {OPT_XBF, "xbf", "REGT_XBF", 1, P_INT, nullptr, C_BOOL},
    {OPT_FUSED_BWD, "fused_bwd", "REGT_FUSED_BWD", 1, P_INT, nullptr, C_BOOL},
    {OPT_TGCN_COLLAPSE, "tgcn_collapse", "REGT_TGCN_COLLAPSE", 1, P_INT, nullptr, C_BOOL},
    {OPT_DGRAD1_GEN, "dgrad1_gen", "REGT_DGRAD1_GEN", 1, P_INT, nullptr, C_BOOL},
    {OPT_SPMM_ROWS, "spmm_rows", "REGT_SPMM_ROWS", 0, P_INT, nullptr, C_BOOL},          // opt-in: measured slower
    {OPT_FUSED_ROWS, "fused_rows", nullptr, 1, P_INT, nullptr, C_ROWS},
    {OPT_EMBED_KERNEL, "embed_kernel", nullptr, 1, P_INT, nullptr, C_BOOL},
    {OPT_WGRAD_RING, "wgrad_ring", nullptr, 6, P_INT, nullptr, C_NONNEG},
    {OPT_WGRAD_TILE, "wgrad_tile", nullptr, 256, P_INT, nullptr, C_TILE},
    {OPT_WGRAD_RING256, "wgrad_ring256", nullptr, 2, P_INT, nullptr, C_RING256},
    {OPT_WGRAD_BNW64, "wgrad_bnw64", nullptr, 1, P_INT, nullptr, C_BOOL},
    {OPT_WGRAD_WAVE, "wgrad_wave", nullptr, 1, P_INT, nullptr, C_BOOL},
    {OPT_WGRAD_PAIRS, "wgrad_pairs", nullptr, 2, P_INT, nullptr, C_PAIRS},
    {OPT_GEMM_MODE, nullptr, "REGT_GEMM_MODE", 0, P_MODE, nullptr, C_MODE},              // set at run time by regt_set_gemm_mode
    {OPT_FP32_CORE, nullptr, "REGT_FP32_CORE", 0, P_WORD, "wide", C_NONE},
    {OPT_GEMM_DESC, nullptr, "REGT_GEMM_DESC", 0, P_WORD, "table", C_NONE},
    {OPT_HIPGRAPH, nullptr, "REGT_HIPGRAPH", 0, P_INT, nullptr, C_NONE},                 // 0 off, 1 small problems only, 2 always
    {OPT_SIDE_STREAM, nullptr, "REGT_SIDE_STREAM", 1, P_INT, nullptr, C_NONE},
    {OPT_SPMM_PL, nullptr, "REGT_SPMM_PL", 0, P_INT, nullptr, C_NONE},                   // 8 | 16 forces a panel width
    {OPT_FUSED_TRACE, nullptr, "REGT_FUSED_TRACE", 0, P_INT, nullptr, C_NONE},           // 1 forward, 2 backward kernel
};
constexpr bool rows_in_enum_order() {
    for (int i = 0; i < OPT_COUNT; ++i)
        if (ROWS[i].id != i) return false;
    return true;
}
static_assert(sizeof(ROWS) / sizeof(ROWS[0]) == OPT_COUNT && rows_in_enum_order(), "ROWS must list every OptId once, in order");

constexpr int UNREAD = INT_MIN;
struct Slot { std::atomic<int> v{UNREAD}; };
Slot g_slots[OPT_COUNT];

int parse(const Row& r, const char* e) {
    switch (r.parse) {
        case P_WORD: return !strcmp(e, r.word) ? 1 : 0;
        case P_MODE: return !strcmp(e, "bf16x3") || !strcmp(e, "1") ? 1 : !strcmp(e, "bf16") || !strcmp(e, "2") ? 2 : 0;
        default: return atoi(e);
    }
}
int clamp(Clamp c, int v) {
    switch (c) {
        case C_BOOL: return v ? 1 : 0;
        case C_ROWS: return v == 2 ? 2 : (v ? 1 : 0);
        case C_NONNEG: return v < 0 ? 0 : v;
        case C_TILE: return v == 256 ? 256 : 128;
        case C_RING256: return v == 4 ? 4 : 2;
        case C_PAIRS: return v < 0 || v > 2 ? 2 : v;
        case C_MODE: return v == 1 || v == 2 ? v : 0;
        default: return v;
    }
}

}  // namespace

int option(OptId id) {
    std::atomic<int>& s = g_slots[id].v;
    int v = s.load(std::memory_order_relaxed);
    if (v != UNREAD) return v;
    const Row& r = ROWS[id];
    const char* e = r.env ? getenv(r.env) : nullptr;
    const int first = e ? clamp(r.clamp, parse(r, e)) : r.dflt;
    return s.compare_exchange_strong(v, first, std::memory_order_relaxed) ? first : v;      // (a value set meanwhile wins)
}

int set_option(OptId id, int value) {
    const int prev = option(id);
    g_slots[id].v.store(clamp(ROWS[id].clamp, value), std::memory_order_relaxed);
    return prev;
}

int set_option(const char* name, int value) {
    for (const Row& r : ROWS)
        if (r.name && !strcmp(name, r.name)) return set_option(r.id, value);
    set_error("regt_set_option: unknown option '%s'", name);
    return -1;
}

}  // namespace regt
