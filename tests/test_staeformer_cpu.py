"""STAEformer without a GPU: the restatement against the reference module's eval-mode goldens (output and the run.py / predict.py
metrics), the module's state_dict layout and seeded initialisation, the refusals, the command-line switch, the four new symbols
of the C ABI and the host-side validation of every limit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_npz
from staeformer_math import add_layernorm, attention, decode_bf16, encode_bf16, golden_state_dict, staeformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["in6_out1", "in12_out3_b2"]
NKEYS = {"in6_out1": 102, "in12_out3_b2": 38}
# the largest gap between staeformer_math in float64 and the reference module's recorded fp32 output (one thread), as
# tools/make_staeformer_goldens.py printed it when it wrote the files: 5.05e-7 (in6_out1), 7.71e-7 (in12_out3_b2), at output
# magnitudes 0.87 and 1.04
GAP = 8e-7
SYMBOLS = ["regt_stae_sizes", "regt_stae_forward", "regt_stae_attention", "regt_stae_add_layernorm"]


def _golden(tag):
    g = load_npz(f"golden_staeformer_{tag}.npz")
    return g, golden_state_dict(g)


def _module(g, **kw):
    import regtgcn_amd as R
    return R.STAEformer(num_nodes=int(g["nodes"]), in_steps=int(g["t_in"]), out_steps=int(g["t_out"]), tod_embedding_dim=0,
                        num_layers=int(g["num_layers"]), **kw)


def test_module_is_exported():
    import regtgcn_amd as R
    assert issubclass(R.STAEformer, torch.nn.Module) and "STAEformer" in R.__all__


def test_byte_planes_round_trip():
    t = torch.randn(3, 5).to(torch.bfloat16).to(torch.float32)
    assert torch.equal(decode_bf16(encode_bf16(t)), t)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_eval_golden_and_metrics(tag):
    g, params = _golden(tag)
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    assert {0, 1} <= set(x[..., 2].long().unique().tolist())              # both rows of dow_embedding are read
    with torch.no_grad():
        o32 = staeformer(params, x, int(g["t_out"]), dtype=torch.float32)
        o64 = staeformer(params, x, int(g["t_out"]))
    assert o32.dtype == torch.float32 and tuple(o32.shape) == tuple(g["eval__out"].shape)
    gap = float((o64 - torch.from_numpy(g["eval__out"]).double()).abs().max())
    print(f"{tag}: float64 restatement vs the reference's fp32 output {gap:.3g}, fp32 restatement "
          f"{float((o32 - torch.from_numpy(g['eval__out'])).abs().max()):.3g}")
    assert gap <= GAP
    np.testing.assert_allclose(o32.numpy(), g["eval__out"], atol=1e-5)
    ae, se, ape = [], [], []
    for k in range(x.shape[0]):
        assert abs(((o64[k][0] - y[k].double()) ** 2).mean().item() - g["eval__test_mse"][k]) < 1e-5
        err = (y[k].double() - o64[k:k + 1]).numpy()
        ae.append(np.abs(err)), se.append(err ** 2), ape.append(np.abs(err) / np.percentile(y[k].numpy(), q=95))
    assert abs(np.concatenate(ae).mean() - g["eval__mae"][0]) < 1e-5
    assert abs(np.concatenate(se).mean() - g["eval__mse"][0]) < 1e-5
    assert abs(np.concatenate(ape).mean() * 100 - g["eval__mape"][0]) < 1e-3


def test_restated_ops_agree_with_torch():
    """attention and add_layernorm of the restatement against torch's own scaled_dot_product_attention and layer_norm."""
    gen = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(2, 5, 7, 64, generator=gen, dtype=torch.float64) for _ in range(3))
    for axis in (1, 2):
        def split(z):
            z = z.transpose(1, 2) if axis == 1 else z
            return z.reshape(z.shape[0], z.shape[1], z.shape[2], 2, 32).transpose(2, 3)
        o = torch.nn.functional.scaled_dot_product_attention(split(q), split(k), split(v))
        o = o.transpose(2, 3).reshape(2, o.shape[1], o.shape[3], 64)
        o = o.transpose(1, 2) if axis == 1 else o
        assert float((attention(q, k, v, axis) - o).abs().max()) < 1e-12
    r, y, gm, bt = (torch.randn(*s, generator=gen, dtype=torch.float64) for s in ((9, 64), (9, 64), (64,), (64,)))
    ref = torch.nn.functional.layer_norm(r + y, (64,), gm, bt, 1e-5)
    assert float((add_layernorm(r, y, gm, bt) - ref).abs().max()) < 1e-12


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_layout_and_seeded_init_match_reference(tag):
    g, params = _golden(tag)
    torch.manual_seed(int(g["seed"]))
    mod = _module(g)
    sd = mod.state_dict()
    keys = list(params)
    assert list(sd.keys()) == keys and len(keys) == NKEYS[tag]
    for k, v in params.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    assert [k for k, _ in mod.named_parameters()] == keys
    np.testing.assert_array_equal(sd["adaptive_embedding"][0].numpy(), g["init__adaptive_embedding_t0"])     # xavier-uniform
    np.testing.assert_array_equal(sd["input_proj.weight"].numpy(), g["init__input_proj.weight"])             # torch's default
    mod.load_state_dict(params, strict=True)
    table = mod.param_table()
    assert len(table) == 8 + 32 * int(g["num_layers"]) and [t for t in table if t is not None][0] is mod.adaptive_embedding
    assert [id(t) for t in table if t is not None] == [id(p) for p in mod.parameters()]                      # state_dict order


def test_constructor_signature_is_the_reference_one():
    import inspect
    import regtgcn_amd as R
    sig = inspect.signature(R.STAEformer.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [
        ("in_steps", 12), ("out_steps", 12), ("steps_per_day", 288), ("days_per_week", 7), ("input_dim", 3), ("output_dim", 1),
        ("input_embedding_dim", 24), ("tod_embedding_dim", 24), ("dow_embedding_dim", 24), ("spatial_embedding_dim", 0),
        ("adaptive_embedding_dim", 80), ("feed_forward_dim", 256), ("num_heads", 4), ("num_layers", 3), ("dropout", 0.1),
        ("use_mixed_proj", True)]
    assert list(sig.parameters)[1] == "num_nodes"


def test_constructor_refusals_and_cpu_input():
    import regtgcn_amd as R
    with pytest.raises(NotImplementedError, match="head width"):
        R.STAEformer(10)                                          # the class default: model_dim 152, head width 38
    ok = dict(tod_embedding_dim=0)
    for bad in (dict(num_heads=8), dict(feed_forward_dim=100), dict(feed_forward_dim=2048), dict(in_steps=256), dict(num_layers=9),
                dict(num_layers=0), dict(out_steps=65), dict(use_mixed_proj=False), dict(adaptive_embedding_dim=240, num_heads=9),
                dict(adaptive_embedding_dim=81)):
        with pytest.raises(NotImplementedError, match="head width"):
            R.STAEformer(10, **{**ok, **bad})
    mod = R.STAEformer(10, in_steps=6, out_steps=1, **ok)
    assert mod.model_dim == 128 and len(mod.state_dict()) == 102
    assert R.STAEformer(10, spatial_embedding_dim=32, adaptive_embedding_dim=48, **ok).model_dim == 128
    assert "tod_embedding.weight" in R.STAEformer(10, tod_embedding_dim=32, adaptive_embedding_dim=48).state_dict()
    with pytest.raises(R.RegtError):
        mod.eval()(torch.zeros(1, 6, 10, 8))


def test_tensor_tables_are_checked_before_any_launch():
    import regtgcn_amd as R
    from regtgcn_amd import ops
    mod = R.STAEformer(10, in_steps=6, out_steps=2, tod_embedding_dim=0, num_layers=1)
    dims = mod.dims(2, 8)
    params = mod.param_table()
    with pytest.raises(R.RegtError, match="on cuda:0"):                 # module never moved to the GPU
        ops.stae_check_tables(dims, torch.device("cuda:0"), params)
    cpu = torch.device("cpu")
    ops.stae_check_tables(dims, cpu, params)
    for bad in (lambda t: t.double(), lambda t: torch.zeros(tuple(t.shape) + (2,))[..., 0], lambda t: t.reshape(-1, 1, 1)):
        for i in (1, 2, 8, 20, 39):
            p2 = list(params)
            p2[i] = bad(params[i].detach())
            with pytest.raises(R.RegtError):
                ops.stae_check_tables(dims, cpu, p2)
    with pytest.raises(R.RegtError):                                     # a time-of-day table where the dims say its width is 0
        ops.stae_check_tables(dims, cpu, params[:4] + [torch.zeros(288, 24)] + params[5:])
    with pytest.raises(R.RegtError):
        ops.stae_check_tables(dims, cpu, params[:-1])


def test_parser_accepts_staeformer_for_evaluation_only():
    import regtgcn_amd as R
    b = R.evaluate.build_parser().parse_args(["--model", "STAEformer", "--checkpoint", "c.pt"])
    assert b.model == "STAEformer"
    assert "STAEformer" not in R.train.MODELS                            # training is not offered
    assert callable(R.evaluate.predict_metrics_staeformer)


def test_new_symbols_are_exported_and_match_signatures_and_header():
    import regtgcn_amd as R
    from regtgcn_amd import _lib
    lib = R.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "regtgcn.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        decl = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert decl, f"{name} is not declared in include/regtgcn.h"
        assert res is ctypes.c_int32 and len(args) == len(decl.group(1).split(",")), name
    fields = re.search(r"typedef struct \{([^}]*)\}\s*regt_stae_dims;", src, flags=re.S).group(1)
    names = [n.strip() for part in fields.split(";") for n in re.sub(r"\b(int32_t|float)\b", "", part).split(",") if n.strip()]
    assert names == [n for n, _ in _lib.StaeDims._fields_]
    assert lib.regt_abi_version() == _lib.ABI_VERSION == 8


def _dims(**kw):
    from regtgcn_amd import _lib
    d = dict(batch=1, in_steps=6, num_nodes=104, in_features=8, input_dim=3, input_embedding_dim=24, tod_embedding_dim=0,
             dow_embedding_dim=24, spatial_embedding_dim=0, adaptive_embedding_dim=80, steps_per_day=288, days_per_week=7, num_heads=4,
             feed_forward_dim=256, num_layers=3, out_steps=1, output_dim=1, use_mixed_proj=1, ln_eps=1e-5)
    d.update(kw)
    return _lib.StaeDims(*d.values())


def test_sizes_accepts_the_contract_and_rejects_every_limit():
    import regtgcn_amd as R
    lib = R.load_library()
    ws = ctypes.c_size_t()
    assert lib.regt_stae_sizes(ctypes.byref(_dims()), ctypes.byref(ws)) == 0
    assert ws.value == 6 * 104 * (6 * 128 + 256)                        # two activations, Q|K|V, attention output, hidden
    assert lib.regt_stae_sizes(ctypes.byref(_dims(adaptive_embedding_dim=208, num_heads=8, feed_forward_dim=1024, in_steps=255, num_layers=8,
                                                  out_steps=64, in_features=256, input_dim=256)), ctypes.byref(ws)) == 0
    for bad, word in ((dict(num_heads=8), b"head width"),                                        # 128 / 8 = 16
                      (dict(adaptive_embedding_dim=81), b"model_dim"),                           # 129: no multiple of 32
                      (dict(adaptive_embedding_dim=240, num_heads=9), b"model_dim"),             # 288 > 256
                      (dict(feed_forward_dim=100), b"feed_forward_dim"), (dict(feed_forward_dim=1056), b"feed_forward_dim"),
                      (dict(in_steps=0), b"in_steps"), (dict(in_steps=256), b"in_steps"),
                      (dict(num_layers=0), b"num_layers"), (dict(num_layers=9), b"num_layers"),
                      (dict(input_dim=9), b"input_dim"), (dict(in_features=257), b"in_features"), (dict(in_features=2), b"in_features"),
                      (dict(out_steps=65), b"out_steps * output_dim"), (dict(out_steps=13, output_dim=5), b"out_steps * output_dim"),
                      (dict(use_mixed_proj=0), b"use_mixed_proj"), (dict(batch=0), b"batch"), (dict(num_nodes=0), b"num_nodes"),
                      (dict(ln_eps=0.0), b"ln_eps")):
        assert lib.regt_stae_sizes(ctypes.byref(_dims(**bad)), ctypes.byref(ws)) != 0, bad
        assert word in lib.regt_last_error(), (bad, lib.regt_last_error())
    assert lib.regt_stae_sizes(None, ctypes.byref(ws)) != 0 and b"dims is NULL" in lib.regt_last_error()


def test_entry_points_validate_on_the_host():
    """NULL tables, misaligned or too narrow rows, a wrong axis and a bad width are refused before anything touches a GPU."""
    import regtgcn_amd as R
    lib = R.load_library()
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 15) & ~15
    d = ctypes.byref(_dims())
    null_table = (ctypes.c_void_p * 128)()
    full = (ctypes.c_void_p * 128)(*([p] * 128))
    assert lib.regt_stae_forward(d, p, null_table, p, p, None) != 0 and b"NULL" in lib.regt_last_error()
    assert lib.regt_stae_forward(d, p, None, p, p, None) != 0 and b"NULL" in lib.regt_last_error()
    assert lib.regt_stae_forward(d, None, full, p, p, None) != 0 and b"NULL" in lib.regt_last_error()
    assert lib.regt_stae_forward(d, p, full, p, p + 4, None) != 0 and b"aligned" in lib.regt_last_error()
    assert lib.regt_stae_forward(ctypes.byref(_dims(num_layers=9)), p, full, p, p, None) != 0 and b"num_layers" in lib.regt_last_error()
    att = lambda q=p, ld=384, heads=4, axis=1, ldo=128, b=1: lib.regt_stae_attention(q, p, p, ld, b, 6, 104, heads, axis, p, ldo, None)
    assert att(q=None) != 0 and b"NULL" in lib.regt_last_error()
    assert att(axis=0) != 0 and b"axis" in lib.regt_last_error()
    assert att(axis=3) != 0 and b"axis" in lib.regt_last_error()
    assert att(heads=9) != 0 and b"heads" in lib.regt_last_error()
    assert att(ld=127) != 0 and b"ld" in lib.regt_last_error()
    assert att(ld=386) != 0 and b"multiples of 4" in lib.regt_last_error()
    assert att(ldo=64) != 0 and b"ldo" in lib.regt_last_error()
    assert att(q=p + 4) != 0 and b"aligned" in lib.regt_last_error()
    assert att(b=0) != 0 and b"batch" in lib.regt_last_error()
    ln = lambda m=10, dd=128, eps=1e-5, r=p: lib.regt_stae_add_layernorm(r, p, p, p, eps, m, dd, p, None)
    assert ln(r=None) != 0 and b"NULL" in lib.regt_last_error()
    assert ln(dd=48) != 0 and b"multiple of 32" in lib.regt_last_error()
    assert ln(dd=288) != 0 and b"multiple of 32" in lib.regt_last_error()
    assert ln(m=0) != 0 and b"M must be" in lib.regt_last_error()
    assert ln(eps=0.0) != 0 and b"eps" in lib.regt_last_error()
