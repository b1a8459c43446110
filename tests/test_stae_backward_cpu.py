"""The STAEformer self-attention layer's backward without a GPU: the new symbols of the C ABI and the host-side validation of every
new entry, nn.SelfAttentionLayer's constructor, state_dict layout and refusals, the restatement with autograd against the reference's
recorded output and gradients, and the conditioning of every case the GPU tests use."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import load_npz
from grad_bars import ill_conditioned
from stae_layer_bars import (ATTN_CASES, LARGE_SCORE_CASES, LAYER_3D_SHAPE, LAYER_SHAPES, LN_CASES, attention_case, attention_grad_dicts,
                             block_rows, layer_case, layer_state, layernorm_case, layernorm_grad_dicts, stack_case, stack_layer_grads)
from stae_layer_math import LAYER_KEYS, key_bias_scale, layer_grads
from staeformer_math import golden_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the largest gap between stae_layer_math in float64 and the reference layer's recorded fp32 output and 17 gradients (one thread), as
# tools/make_stae_layer_goldens.py printed it when it wrote the file: 6.81e-6 (a weight gradient of magnitude ~30)
GAP = 7e-6
SYMBOLS = {"regt_stae_attention_train": 13, "regt_stae_attention_backward_scratch_floats": 4, "regt_stae_attention_backward": 19,
           "regt_stae_add_layernorm_backward_scratch_floats": 2, "regt_stae_add_layernorm_backward": 12}


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_bound_and_declared():
    import regtgcn_amd as R
    from regtgcn_amd import _lib
    lib = R.load_library()
    src = open(os.path.join(ROOT, "include", "regtgcn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in SYMBOLS.items():
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, src)
        assert m, f"{name} is not declared in include/regtgcn.h"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
    assert lib.regt_abi_version() == _lib.ABI_VERSION == 8


def _err(lib):
    return lib.regt_last_error().decode()


def test_attention_entries_validate_on_the_host():
    import regtgcn_amd as R
    lib = R.load_library()
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)           # never dereferenced: every call below is refused before a launch

    def train(q=one, ld=128, b=2, t=5, n=7, heads=4, axis=1, out=one, ldo=128, lse=one):
        return lib.regt_stae_attention_train(q, one, one, ld, b, t, n, heads, axis, out, ldo, lse, None)

    def bwd(q=one, ld=128, ldo=128, lse=one, b=2, t=5, n=7, heads=4, axis=1, dq=one, ldg=128, scratch=one):
        return lib.regt_stae_attention_backward(q, one, one, ld, one, one, ldo, lse, b, t, n, heads, axis, dq, one, one, ldg, scratch, None)

    for call in (train, bwd):
        assert call(q=None) != 0 and "NULL" in _err(lib)
        assert call(lse=None) != 0 and "NULL" in _err(lib)
        assert call(q=odd) != 0 and "16-byte aligned" in _err(lib)
        assert call(lse=odd) != 0 and "16-byte aligned" in _err(lib)
        assert call(ld=130) != 0 and "multiples of 4" in _err(lib)
        assert call(ld=124) != 0 and "at least 32 * heads" in _err(lib)
        assert call(ldo=64) != 0 and "at least 32 * heads" in _err(lib)
        assert call(axis=0) != 0 and "axis must be 1" in _err(lib)
        assert call(axis=3) != 0 and "axis must be 1" in _err(lib)
        assert call(heads=0) != 0 and "heads must be in [1, 8]" in _err(lib)
        assert call(heads=9, ld=288, ldo=288) != 0 and "heads must be in [1, 8]" in _err(lib)
        assert call(b=0) != 0 and "must be >= 1" in _err(lib)
        assert call(b=1 << 15, t=1 << 7, n=1 << 7) != 0 and "too large" in _err(lib)
    assert train(out=None) != 0 and "NULL" in _err(lib)
    assert bwd(dq=None) != 0 and "NULL" in _err(lib)
    assert bwd(scratch=None) != 0 and "NULL" in _err(lib)
    assert bwd(dq=odd) != 0 and "16-byte aligned" in _err(lib)
    assert bwd(ldg=126) != 0 and "multiples of 4" in _err(lib)
    assert bwd(ldg=96) != 0 and "at least 32 * heads" in _err(lib)
    assert lib.regt_stae_attention_backward_scratch_floats(2, 5, 7, 4) == 2 * 5 * 7 * 4
    assert lib.regt_stae_attention_backward_scratch_floats(2, 5, 7, 9) == 0 and "heads must be in [1, 8]" in _err(lib)
    assert lib.regt_stae_attention_backward_scratch_floats(1 << 15, 1 << 7, 1 << 7, 4) == 0 and "too large" in _err(lib)


def test_add_layernorm_backward_validates_on_the_host():
    import regtgcn_amd as R
    lib = R.load_library()
    a = [ctypes.c_void_p(256 * (i + 1)) for i in range(8)]          # distinct, 16-byte aligned, never dereferenced
    odd = ctypes.c_void_p(260)

    def bwd(res=a[0], gamma=a[2], eps=1e-5, m=10, d=128, dz=a[4], scratch=a[7]):
        return lib.regt_stae_add_layernorm_backward(res, a[1], gamma, a[3], eps, m, d, dz, a[5], a[6], scratch, None)

    assert bwd(res=None) != 0 and "NULL" in _err(lib)
    assert bwd(scratch=None) != 0 and "NULL" in _err(lib)
    assert bwd(gamma=odd) != 0 and "16-byte aligned" in _err(lib)
    assert bwd(dz=odd) != 0 and "16-byte aligned" in _err(lib)
    for d in (0, 16, 48, 288):
        assert bwd(d=d) != 0 and "D must be a multiple of 32 in [32, 256]" in _err(lib)
    assert bwd(eps=0.0) != 0 and "eps must be > 0" in _err(lib)
    assert bwd(m=0) != 0 and "M must be in [1, 2^31 / 4)" in _err(lib)
    assert bwd(m=1 << 29) != 0 and "M must be in [1, 2^31 / 4)" in _err(lib)
    assert bwd(dz=a[0]) != 0 and "must not alias" in _err(lib)
    assert lib.regt_stae_add_layernorm_backward_scratch_floats(1000, 128) >= 2 * 128 * (1000 // 64)
    assert lib.regt_stae_add_layernorm_backward_scratch_floats(1000, 48) == 0 and "D must be" in _err(lib)
    assert lib.regt_stae_add_layernorm_backward_scratch_floats(1 << 29, 128) == 0 and "M must be" in _err(lib)


# ---- the module ---------------------------------------------------------------------------------------------------------------------

def test_layer_constructor_forward_and_state_dict_are_the_reference_ones():
    import regtgcn_amd as R
    assert issubclass(R.SelfAttentionLayer, torch.nn.Module) and "SelfAttentionLayer" in R.__all__
    sig = inspect.signature(R.SelfAttentionLayer.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("model_dim", inspect.Parameter.empty), ("feed_forward_dim", 2048), ("num_heads", 8), ("dropout", 0), ("mask", False)]
    fsig = inspect.signature(R.SelfAttentionLayer.forward)
    assert [(k, v.default) for k, v in list(fsig.parameters.items())[1:]] == [("x", inspect.Parameter.empty), ("dim", -2)]
    g = load_npz("golden_stae_layer.npz")
    want = golden_state_dict(g)
    assert list(want) == LAYER_KEYS
    mod = R.SelfAttentionLayer(int(g["model_dim"]), feed_forward_dim=int(g["feed_forward_dim"]), num_heads=int(g["num_heads"]))
    sd = mod.state_dict()
    assert list(sd) == list(want) == [k for k, _ in mod.named_parameters()]
    assert all(tuple(sd[k].shape) == tuple(want[k].shape) for k in want)
    mod.load_state_dict(want, strict=True)
    assert list(layer_state()) == LAYER_KEYS


def test_layer_refusals():
    import regtgcn_amd as R
    with pytest.raises(NotImplementedError, match="head width"):
        R.SelfAttentionLayer(152, feed_forward_dim=256, num_heads=4)             # STAEformer's class default: head width 38
    with pytest.raises(NotImplementedError, match="head width"):
        R.SelfAttentionLayer(128, feed_forward_dim=256, num_heads=8)
    with pytest.raises(NotImplementedError, match="model_dim <= 256"):
        R.SelfAttentionLayer(288, feed_forward_dim=256, num_heads=9)
    for ff in (2048, 100, 16):                                                   # the reference's default 2048 is over the limit
        with pytest.raises(NotImplementedError, match="feed_forward_dim"):
            R.SelfAttentionLayer(128, feed_forward_dim=ff, num_heads=4)
    with pytest.raises(NotImplementedError, match="feed_forward_dim"):
        R.SelfAttentionLayer(256)
    with pytest.raises(NotImplementedError, match="mask"):
        R.SelfAttentionLayer(128, 256, 4, 0, True)
    mod = R.SelfAttentionLayer(128, 256, 4, dropout=0.1)                         # constructs: eval() runs it
    assert mod.training and mod.dropout == pytest.approx(0.1)
    with pytest.raises(NotImplementedError, match="dropout"):                    # training mode would draw masks: refused before the device check
        mod(torch.zeros(2, 5, 7, 128))
    with pytest.raises(NotImplementedError, match="dropout"):
        mod(torch.zeros(2, 7, 128), dim=1)
    with pytest.raises(R.RegtError):                                             # eval(): dropout is the identity, the call gets as far as the device check
        mod.eval()(torch.zeros(2, 5, 7, 128))
    with pytest.raises(R.RegtError):
        R.SelfAttentionLayer(128, 256, 4)(torch.zeros(2, 5, 7, 128))             # CPU tensor
    with pytest.raises(R.RegtError):
        R.SelfAttentionLayer(128, 256, 4)(torch.zeros(2, 7, 128), dim=1)


# ---- the restatement against the reference's recorded numbers ---------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 2])
def test_restatement_reproduces_golden_output_and_gradients(dim):
    g = load_npz("golden_stae_layer.npz")
    sd = golden_state_dict(g)
    x, dout = torch.from_numpy(g["x"]), torch.from_numpy(g["dout"])
    assert tuple(x.shape) == (2, 5, 7, 64) and float(dout.std(dim=(0, 1, 2)).min()) > 0 and dout.unique().numel() > dout.numel() // 2
    for k, v in sd.items():                                                      # perturbed away from the 0 / 1 initial values
        if k.endswith("bias") or k.startswith("ln"):
            assert float((v - (1.0 if k in ("ln1.weight", "ln2.weight") else 0.0)).abs().max()) > 0.05, k
    o64, g64 = layer_grads(sd, x, dim, dout)
    assert list(g64) == ["x"] + LAYER_KEYS
    worst = float((o64 - torch.from_numpy(g[f"dim{dim}__out"]).double()).abs().max())
    assert worst <= GAP + 1e-5
    for k, v in g64.items():
        gap = float((v - torch.from_numpy(g[f"dim{dim}__grad__{k}"]).double()).abs().max())
        worst = max(worst, gap)
        assert gap <= GAP + 1e-5, (k, gap)
    print(f"golden layer dim {dim}: float64 restatement vs the reference's fp32 numbers, worst of 18 tensors {worst:.3g}")


# ---- conditioning, decided by the references alone (the fp32 restatement stands in for the kernels) ----------------------------------------

def _ill(rows):
    return [label for label, cls, err, scale, gap in rows if ill_conditioned(cls, scale, gap)]


@pytest.mark.parametrize("dim", [1, 2])
def test_no_golden_block_is_ill_conditioned(dim):
    g = load_npz("golden_stae_layer.npz")
    sd = golden_state_dict(g)
    x, dout = torch.from_numpy(g["x"]), torch.from_numpy(g["dout"])
    _, g64 = layer_grads(sd, x, dim, dout)
    ref = {k: torch.from_numpy(g[f"dim{dim}__grad__{k}"]) for k in g64}
    scales = {"attn.FC_K.bias": key_bias_scale(sd, x, dim, dout)}
    assert float(g64["attn.FC_K.bias"].abs().max()) < 1e-12 < 1e-3 < scales["attn.FC_K.bias"]       # identically zero: residue only
    rows = block_rows(ref, g64, ref, scales=scales)
    assert len(rows) == 2 + 4 * 4 + 4 + 4 + 4 + 2 + 4 and not _ill(rows), _ill(rows)
    _, g32 = layer_grads(sd, x, dim, dout, dtype=torch.float32)
    assert not _ill(block_rows(g32, g64, g32, scales=scales))


def test_at_most_five_percent_of_the_gpu_files_blocks_are_ill_conditioned():
    """Every gradient comparison of tests/test_gpu_stae_backward.py: the op-level cases, the layer cases, the (B, L, D) case and the
    two-layer stack (the golden has a test of its own above).  This test needs nothing of the library: it is about the cases."""
    total, ill = 0, []
    b3, n3 = LAYER_3D_SHAPE
    case, r64, r32 = layer_case(b3, 1, n3, 2)
    rows = block_rows(r32[1], r64[1], r32[1], scales=case["scales"])
    total, ill = total + len(rows), ill + [f"layer on (B, L, D): {l}" for l in _ill(rows)]
    case, (_, g64), (_, g32) = stack_case()
    for i in (0, 1):
        rows = block_rows(stack_layer_grads(g32, i), stack_layer_grads(g64, i), stack_layer_grads(g32, i), scales=case["scales"][i])
        total, ill = total + len(rows), ill + [f"two-layer stack, layer {i}: {l}" for l in _ill(rows)]
    rows = block_rows({"x": g32["x"]}, {"x": g64["x"]}, {"x": g32["x"]})
    total, ill = total + len(rows), ill + [f"two-layer stack: {l}" for l in _ill(rows)]
    for length, axis, heads, batch in ATTN_CASES:
        _, r64, r32 = attention_case(length, axis, heads, batch)
        rows = block_rows(attention_grad_dicts(r32), attention_grad_dicts(r64), attention_grad_dicts(r32), axis)
        total, ill = total + len(rows), ill + [f"attention L {length} axis {axis} heads {heads} B {batch}: {l}" for l in _ill(rows)]
    for length, axis, heads, batch in LARGE_SCORE_CASES:
        _, r64, r32 = attention_case(length, axis, heads, batch, 30.0)
        rows = block_rows(attention_grad_dicts(r32), attention_grad_dicts(r64), attention_grad_dicts(r32), axis)
        total, ill = total + len(rows), ill + [f"attention q x 30 axis {axis}: {l}" for l in _ill(rows)]
    for m, d, kind in [(m, d, "normal") for m, d in LN_CASES] + [(65, 32, "constant_row"), (65, 256, "constant_row"), (65, 128, "gamma_zeros")]:
        _, r64, r32 = layernorm_case(m, d, kind)
        rows = block_rows(layernorm_grad_dicts(r32), layernorm_grad_dicts(r64), layernorm_grad_dicts(r32))
        total, ill = total + len(rows), ill + [f"add_layernorm M {m} D {d} {kind}: {l}" for l in _ill(rows)]
    for b, t, n in LAYER_SHAPES:
        for axis in (1, 2):
            case, r64, r32 = layer_case(b, t, n, axis)
            rows = block_rows(r32[1], r64[1], r32[1], scales=case["scales"])
            total, ill = total + len(rows), ill + [f"layer B {b} T {t} N {n} axis {axis}: {l}" for l in _ill(rows)]
    print(f"{total} blocks, {len(ill)} ill-conditioned ({100.0 * len(ill) / total:.2f} %)" + "".join("\n  " + l for l in ill[:30]))
    assert total > 3000 and len(ill) <= 0.05 * total, (len(ill), total)
