// The process-wide switches of the library: which kernels run for the same arithmetic (A/B timing, and the bit-for-bit comparisons
// of the test suite).  One table in options.hip holds every switch's regt_set_option name, environment variable, default and
// normalisation; it is the only place of the library that reads the environment.  What each switch selects is documented where
// it is used and in include/regtgcn.h / DESIGN.md section 6b.
#pragma once

namespace regt {

enum OptId : int {
    OPT_XBF, OPT_FUSED_BWD, OPT_TGCN_COLLAPSE, OPT_DGRAD1_GEN, OPT_SPMM_ROWS, OPT_FUSED_ROWS, OPT_EMBED_KERNEL,
    OPT_WGRAD_RING, OPT_WGRAD_TILE, OPT_WGRAD_RING256, OPT_WGRAD_BNW64, OPT_WGRAD_WAVE, OPT_WGRAD_PAIRS,
    OPT_GEMM_MODE, OPT_FP32_CORE, OPT_GEMM_DESC, OPT_HIPGRAPH, OPT_SIDE_STREAM, OPT_SPMM_PL, OPT_FUSED_TRACE,
    OPT_COUNT
};

// The current value.  The first use of a switch reads its environment variable (not earlier: a process may set the variable after
// loading the library); a value set before that wins.
int option(OptId id);
// Stores `value` as the switch's rule normalises it and returns the previous value.  By name (regt_set_option): -1 and an error
// message for a name that is not in the table or belongs to an environment-only switch.
int set_option(OptId id, int value);
int set_option(const char* name, int value);

}  // namespace regt
