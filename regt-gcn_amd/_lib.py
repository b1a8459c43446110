"""ctypes binding of libregtgcn_hip.so (C ABI: include/regtgcn.h).

There is no fallback: if the library is missing or a call fails, this module raises.
PyTorch is used by the callers only to own device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# REGT_LIB_DIR: a developer build of the same library in another directory (build.py honours the same variable), e.g. the
# workgroup-trace build of tools/wg_trace.py; never a different implementation
LIB_PATH = os.path.join(os.environ.get("REGT_LIB_DIR") or os.path.join(HERE, "lib"), "libregtgcn_hip.so")
ABI_VERSION = 8

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)
vp = C.c_void_p


class RegtError(RuntimeError):
    pass


class Dims(C.Structure):
    _fields_ = [("N", C.c_int32), ("T", C.c_int32), ("F", C.c_int32), ("C", C.c_int32), ("R", C.c_int32),
                ("O", C.c_int32), ("H1", C.c_int32), ("regional", C.c_int32), ("lrelu_slope", C.c_float),
                # ABI v6, per-call configuration (zero = process defaults): GEMM arithmetic (ARITH_*), DIMS_* flag bits
                ("arith", C.c_int32), ("flags", C.c_uint32)]


ARITH_DEFAULT, ARITH_FP32, ARITH_BF16X3, ARITH_BF16 = 0, 1, 2, 3
ARITH_NAMES = {None: ARITH_DEFAULT, "default": ARITH_DEFAULT, "fp32": ARITH_FP32, "bf16x3": ARITH_BF16X3, "bf16": ARITH_BF16}
DIMS_NO_BF16_ROWS, DIMS_NO_FUSED_BWD, DIMS_NO_SIDE_STREAM = 1, 2, 4
DIMS_FORWARD_ONLY = 8      # forward entry points: no backward follows; workspace of regt_forward_only_workspace_bytes
DIMS_NO_HEAD = 16          # regt_forward / regt_backward: the cell alone (pred / dpred may be NULL, dhidden is the whole upstream gradient)


def arith_code(arith) -> int:
    """``None`` / "default" / "fp32" / "bf16x3" / "bf16" (or the REGT_ARITH_* integer) -> regt_dims.arith."""
    if isinstance(arith, int) and not isinstance(arith, bool) and 0 <= arith <= 3:
        return arith
    try:
        return ARITH_NAMES[arith]
    except (KeyError, TypeError):
        raise ValueError(f"arithmetic must be one of {sorted(k for k in ARITH_NAMES if k)} or None, got {arith!r}") from None


class StnormDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_nodes", "batch", "tnorm_group", "seq_len", "in_dim", "out_dim", "blocks", "layers",
                                         "tnorm", "snorm", "training")]


class StidDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_nodes", "batch", "input_len", "in_features", "input_dim", "embed_dim", "node_dim",
                                         "num_layer", "output_len", "if_node")] + [("dropout_p", C.c_float)]


class GruDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("seq_len", "rows", "input_size", "hidden", "training")] + \
               [(n, C.c_int64) for n in ("x_stride_seq", "x_stride_row", "x_stride_t")]


class StaeDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("batch", "in_steps", "num_nodes", "in_features", "input_dim", "input_embedding_dim",
                                         "tod_embedding_dim", "dow_embedding_dim", "spatial_embedding_dim", "adaptive_embedding_dim",
                                         "steps_per_day", "days_per_week", "num_heads", "feed_forward_dim", "num_layers", "out_steps",
                                         "output_dim", "use_mixed_proj")] + [("ln_eps", C.c_float)]


class Graph(C.Structure):
    _fields_ = [("rowptr", vp), ("col", vp), ("val", vp), ("node_region", vp), ("chunk_tab", vp),
                ("chunk_region", vp), ("n_chunks", C.c_int32),
                ("m_rowptr", vp), ("m_col", vp), ("m_val_a", vp), ("m_val_l", vp), ("overlap", C.c_int32),
                ("region_lo", C.c_int32), ("region_hi", C.c_int32), ("region_sorted", C.c_int32)]


_PARAM_FIELDS = [("attention", vp), ("conv_lin_w", vp * 3), ("conv_bias", vp * 3), ("gate_w", vp * 3),
                 ("gate_b", vp * 3), ("cheb_w0", vp), ("cheb_w1", vp), ("cheb_bias", vp), ("region_w", vp),
                 ("region_b", vp), ("head1_w", vp), ("head1_b", vp), ("head2_w", vp), ("head2_b", vp)]


class Params(C.Structure):
    _fields_ = _PARAM_FIELDS


class Grads(C.Structure):
    _fields_ = _PARAM_FIELDS


class Cell0Args(C.Structure):
    _fields_ = [("a_z", vp), ("a_h", vp), ("kz", C.c_int32), ("kh", C.c_int32), ("gz", vp), ("gh", vp), ("cz", vp), ("ch", vp),
                ("attention", vp), ("head1_w", vp), ("head1_b", vp), ("head2_w", vp), ("head2_b", vp)]


class Cell0Grads(C.Structure):
    _fields_ = [("a_z", vp), ("a_h", vp), ("gz", vp), ("gh", vp), ("cz", vp), ("ch", vp), ("attention", vp),
                ("head1_w", vp), ("head1_b", vp), ("head2_w", vp), ("head2_b", vp)]


# name, restype, argtypes -- one entry per function declared in include/regtgcn.h
SIGNATURES = {
    "regt_abi_version": (C.c_int32, []),
    "regt_set_gemm_mode": (C.c_int32, [C.c_int32]),
    "regt_gemm_mode": (C.c_int32, []),
    "regt_set_option": (C.c_int32, [C.c_char_p, C.c_int32]),
    "regt_cell_forward": (C.c_int32, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "regt_cell_backward": (C.c_int32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "regt_tgcn_workspace_bytes": (C.c_size_t, [C.POINTER(Dims)]),
    "regt_tgcn_forward": (C.c_int32, [C.POINTER(Dims), C.POINTER(Graph), C.POINTER(Params), vp, vp, vp, vp, C.c_size_t, vp]),
    "regt_tgcn_backward": (C.c_int32, [C.POINTER(Dims), C.POINTER(Graph), C.POINTER(Params), C.POINTER(Grads), vp, vp, vp, vp, vp, vp,
                                       vp, vp, vp, C.c_size_t, vp]),
    "regt_input_gradient_scratch_bytes": (C.c_size_t, [C.POINTER(Dims)]),
    "regt_input_gradient": (C.c_int32, [C.POINTER(Dims), C.POINTER(Graph), C.POINTER(Params), vp, vp, vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t,
                                        vp]),
    "regt_last_error": (C.c_char_p, []),
    "regt_graph_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "regt_gcn_csr": (C.c_int32, [vp, vp, C.c_int64, C.c_int32, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "regt_gcn_dis": (C.c_int32, [vp, vp, C.c_int64, C.c_int32, vp, vp, vp, C.c_size_t, vp]),
    "regt_cheb_edge_weights": (C.c_int32, [vp, vp, C.c_int64, C.c_int32, vp, vp, vp, C.c_size_t, vp]),
    "regt_raw_csr": (C.c_int32, [vp, vp, C.c_int64, C.c_int32, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "regt_graph_fingerprint": (C.c_int32, [vp, vp, C.c_int64, vp, vp]),
    "regt_spmm_csr": (C.c_int32, [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp]),
    "regt_spmm_dual": (C.c_int32, [vp, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, vp]),
    "regt_pack_x": (C.c_int32, [vp, vp, C.c_int32, C.c_int32, C.c_int32, vp]),
    "regt_pack_x_bf16": (C.c_int32, [vp, vp, C.c_int32, C.c_int32, C.c_int32, vp]),
    "regt_spmm_dual_bf16": (C.c_int32, [vp, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp]),
    "regt_forward_packed_bf16": (C.c_int32, [C.POINTER(Dims), C.POINTER(Graph), C.POINTER(Params), vp, C.c_int32, vp, vp, vp,
                                             C.c_size_t, vp]),
    "regt_linear": (C.c_int32, [vp, C.c_int64, C.c_int64, C.c_int32, vp, C.c_int64, C.c_int32, vp, C.c_int32,
                                C.c_float, vp, C.c_int64, vp]),
    "regt_wgrad_slab_floats": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "regt_wgrad": (C.c_int32, [vp, C.c_int64, vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, vp, C.c_int64, vp, vp, vp]),
    "regt_wgrad_slabs": (C.c_int32, [vp, C.c_int64, C.c_int32, vp, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32,
                                     C.POINTER(C.c_char_p), vp]),
    "regt_workspace_bytes": (C.c_size_t, [C.POINTER(Dims), C.c_int32, C.c_int32]),
    "regt_forward_only_workspace_bytes": (C.c_size_t, [C.POINTER(Dims), C.POINTER(Graph)]),
    "regt_forward_only_packed_workspace_bytes": (C.c_size_t, [C.POINTER(Dims), C.POINTER(Graph), C.c_int32, C.c_int32]),
    "regt_forward": (C.c_int32, [C.POINTER(Dims), C.POINTER(Graph), C.POINTER(Params), vp, vp, vp, vp, C.c_size_t, vp]),
    "regt_forward_packed": (C.c_int32, [C.POINTER(Dims), C.POINTER(Graph), C.POINTER(Params), vp, C.c_int32, vp, vp, vp,
                                        C.c_size_t, vp]),
    "regt_backward": (C.c_int32, [C.POINTER(Dims), C.POINTER(Graph), C.POINTER(Params), C.POINTER(Grads), vp, vp, vp,
                                  vp, vp, C.c_size_t, vp]),
    "regt_window_chunk": (C.c_int32, [C.c_int32]),
    "regt_window_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "regt_window_forward": (C.c_int32, [vp] + [C.c_int32] * 8 + [vp] * 8 + [C.c_size_t, vp]),
    "regt_window_backward_workspace_bytes": (C.c_size_t, [C.c_int32] * 6),
    "regt_window_backward_max_t": (C.c_int32, []),
    "regt_window_backward": (C.c_int32, [vp] + [C.c_int32] * 8 + [vp] * 8 + [C.c_int32] + [vp] * 6 + [C.c_size_t, vp]),
    "regt_mean_csr": (C.c_int32, [vp, C.c_int64, C.c_int32, vp, vp, vp, vp, vp, C.c_size_t, vp]),
    "regt_cell0_workspace_bytes": (C.c_size_t, [C.POINTER(Dims), C.c_int32, C.c_int32]),
    "regt_cell0_forward": (C.c_int32, [C.POINTER(Dims), C.POINTER(Cell0Args), vp, vp, vp, C.c_size_t, vp]),
    "regt_cell0_backward": (C.c_int32, [C.POINTER(Dims), C.POINTER(Cell0Args), C.POINTER(Cell0Grads), vp, vp, vp, vp, C.c_size_t, vp]),
    "regt_gat_forward": (C.c_int32, [vp, vp, vp, vp, vp, C.c_float, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]),
    "regt_gat_backward": (C.c_int32, [vp, vp, vp, vp, vp, vp, C.c_float, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]),
    "regt_graph_stats": (C.c_int32, [C.POINTER(C.c_int64)]),
    "regt_debug_trace": (C.c_int64, [C.POINTER(C.c_int64), C.c_int64]),
    "regt_profile_enable": (C.c_int32, [C.c_int32]),
    "regt_profile_collect": (C.c_int32, [C.c_char_p, C.c_size_t]),
    "regt_spatial_embed_slab_floats": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "regt_spatial_embed_forward": (C.c_int32, [vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]),
    "regt_spatial_embed_backward": (C.c_int32, [vp, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]),
    "regt_stnorm_sizes": (C.c_int32, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "regt_stnorm_forward": (C.c_int32, [vp, vp, vp, vp, vp, vp, vp]),
    "regt_stnorm_backward": (C.c_int32, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "regt_stid_sizes": (C.c_int32, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "regt_stid_forward": (C.c_int32, [vp, vp, vp, vp, vp, vp, vp]),
    "regt_stid_backward": (C.c_int32, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "regt_gru_sizes": (C.c_int32, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "regt_gru_forward": (C.c_int32, [vp] * 11),
    "regt_gru_backward": (C.c_int32, [vp] * 11),
    "regt_stae_sizes": (C.c_int32, [vp, C.POINTER(C.c_size_t)]),
    "regt_stae_forward": (C.c_int32, [vp, vp, vp, vp, vp, vp]),
    "regt_stae_attention": (C.c_int32, [vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int64, vp]),
    "regt_stae_add_layernorm": (C.c_int32, [vp, vp, vp, vp, C.c_float, C.c_int64, C.c_int32, vp, vp]),
    "regt_stae_attention_train": (C.c_int32, [vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int64,
                                              vp, vp]),
    "regt_stae_attention_backward_scratch_floats": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "regt_stae_attention_backward": (C.c_int32, [vp, vp, vp, C.c_int64, vp, vp, C.c_int64, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_int32, vp, vp, vp, C.c_int64, vp, vp]),
    "regt_stae_add_layernorm_backward_scratch_floats": (C.c_size_t, [C.c_int64, C.c_int32]),
    "regt_stae_add_layernorm_backward": (C.c_int32, [vp, vp, vp, vp, C.c_float, C.c_int64, C.c_int32, vp, vp, vp, vp, vp]),
    "regt_stae_embed": (C.c_int32, [vp, vp, vp, vp, vp]),
    "regt_stae_embed_backward_scratch_floats": (C.c_size_t, [vp]),
    "regt_stae_embed_backward": (C.c_int32, [vp, vp, vp, vp, vp, vp]),
    "regt_stae_output_proj": (C.c_int32, [vp, vp, vp, vp, vp, vp]),
    "regt_stae_output_proj_backward_scratch_floats": (C.c_size_t, [vp]),
    "regt_stae_output_proj_backward": (C.c_int32, [vp, vp, vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp, vp, vp, vp, vp]),
    "regt_stae_drop_add_layernorm": (C.c_int32, [vp, vp, vp, C.c_float, vp, vp, C.c_float, C.c_int64, C.c_int32, vp, vp]),
    "regt_stae_drop_add_layernorm_backward_scratch_floats": (C.c_size_t, [C.c_int64, C.c_int32]),
    "regt_stae_drop_add_layernorm_backward": (C.c_int32, [vp, vp, vp, C.c_float, vp, vp, C.c_float, C.c_int64, C.c_int32, vp, vp, vp, vp,
                                                          vp, vp]),
    "regt_relu_backward": (C.c_int32, [vp, vp, C.c_int64, vp]),
    "regt_mse_loss_grad": (C.c_int32, [vp, vp, vp, vp, C.c_int64, C.c_int64, vp]),
}

_lib = None


def load():
    """Load the shared library (once).  Raises RegtError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RegtError(
            f"{LIB_PATH} not found: the HIP library is not built. Run `python regt-gcn_amd/build.py` "
            "(or __graft_entry__.build()). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing -> loud
        fn.restype = res
        fn.argtypes = args
    v = lib.regt_abi_version()
    if v != ABI_VERSION:
        raise RegtError(f"libregtgcn_hip.so ABI version {v} != expected {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().regt_last_error().decode("utf-8", "replace")
        raise RegtError(f"{what} failed (code {rc}): {msg}")


def gemm_mode() -> int:
    """The process default GEMM arithmetic (0 fp32, 1 bf16x3, 2 bf16); reads only."""
    return load().regt_gemm_mode()


def ptr(t):
    """Device pointer of a torch tensor (or None) as a c_void_p value."""
    return None if t is None else C.c_void_p(t.data_ptr())
