"""Whole-STAEformer training, what runs without a GPU: the additive C ABI and its host-side limit checks, the keep-bit draw, the
trainable class's parameters, the parent's refusals, the command's parser, and the conditioning of the GPU file's cases (with the
fp32 restatement in the kernels' place, as tests/test_stae_backward_cpu.py does for the layer)."""
import ctypes
import os
import re

import pytest
import torch

import regtgcn_amd as R
from regtgcn_amd import _lib, nn as rnn, train_staeformer
import staeformer_train_bars as TB
from staeformer_train_math import pack_keep, unpack_keep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["regt_stae_embed", "regt_stae_embed_backward", "regt_stae_embed_backward_scratch_floats", "regt_stae_output_proj",
       "regt_stae_output_proj_backward", "regt_stae_output_proj_backward_scratch_floats", "regt_stae_drop_add_layernorm",
       "regt_stae_drop_add_layernorm_backward", "regt_stae_drop_add_layernorm_backward_scratch_floats"]


def _dims(**over):
    base = dict(batch=2, in_steps=6, num_nodes=33, in_features=8, input_dim=3, input_embedding_dim=24, tod_embedding_dim=0,
                dow_embedding_dim=24, spatial_embedding_dim=0, adaptive_embedding_dim=80, steps_per_day=288, days_per_week=7, num_heads=4,
                feed_forward_dim=256, num_layers=1, out_steps=1, output_dim=1, use_mixed_proj=1, ln_eps=1e-5)
    base.update(over)
    return _lib.StaeDims(*[base[n] for n, _ in _lib.StaeDims._fields_])


def test_new_entries_are_exported_bound_and_abi_stays_8():
    lib = R.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "regtgcn.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, src)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert lib.regt_abi_version() == _lib.ABI_VERSION == 8


def test_host_side_limit_checks_of_every_new_entry():
    lib = R.load_library()
    B, one = ctypes.byref, ctypes.c_void_p(256)
    err = lambda: lib.regt_last_error()
    tab = (ctypes.c_void_p * 8)(*[256] * 8)
    good, bad_heads = _dims(), _dims(num_heads=3)
    assert lib.regt_stae_embed(None, one, tab, one, None) != 0 and b"dims is NULL" in err()
    assert lib.regt_stae_embed(B(bad_heads), one, tab, one, None) != 0 and b"head width" in err()
    assert lib.regt_stae_embed(B(good), None, tab, one, None) != 0 and b"NULL" in err()
    empty = (ctypes.c_void_p * 8)()
    assert lib.regt_stae_embed(B(good), one, empty, one, None) != 0 and b"head entry 1 is NULL" in err()
    assert lib.regt_stae_embed_backward_scratch_floats(B(bad_heads)) == 0 and b"head width" in err()
    assert lib.regt_stae_embed_backward_scratch_floats(B(good)) >= 24 * 4 + 7 * 24
    big = _dims(tod_embedding_dim=96, adaptive_embedding_dim=112, num_heads=8)         # 288 x 96 floats: past one LDS image
    assert lib.regt_stae_embed_backward_scratch_floats(B(big)) == 0 and b"15360" in err()
    assert lib.regt_stae_embed_backward(B(big), one, one, tab, one, None) != 0 and b"LDS" in err()
    assert lib.regt_stae_embed_backward(B(good), one, None, tab, one, None) != 0 and b"NULL" in err()
    assert lib.regt_stae_embed_backward(B(good), one, one, empty, one, None) != 0 and b"gradient entry 1 is NULL" in err()
    assert lib.regt_stae_output_proj(B(_dims(out_steps=65)), one, one, one, one, None) != 0 and b"out_steps * output_dim" in err()
    assert lib.regt_stae_output_proj(B(good), one, None, one, one, None) != 0 and b"NULL" in err()
    assert lib.regt_stae_output_proj_backward_scratch_floats(B(_dims(out_steps=65))) == 0
    assert lib.regt_stae_output_proj_backward_scratch_floats(B(good)) >= 6 * 128 + 1
    assert lib.regt_stae_output_proj_backward(B(good), one, one, None, 1, 1, 1, 1, one, one, one, one, None) != 0 and b"NULL" in err()
    assert lib.regt_stae_output_proj_backward(B(good), one, one, one, -1, 1, 1, 1, None, one, one, one, None) != 0 and b"strides" in err()
    assert lib.regt_stae_output_proj_backward(B(good), one, one, one, 1, 1, 1, 1, one, one, one, one, None) != 0 and b"alias" in err()
    assert lib.regt_stae_drop_add_layernorm(one, one, one, 1.0, one, one, 1e-5, 4, 32, one, None) != 0 and b"[0, 1)" in err()
    assert lib.regt_stae_drop_add_layernorm(one, one, one, 0.1, one, one, 1e-5, 4, 48, one, None) != 0 and b"multiple of 32" in err()
    assert lib.regt_stae_drop_add_layernorm(one, one, one, 0.1, one, one, 1e-5, 0, 32, one, None) != 0 and b"M must be" in err()
    assert lib.regt_stae_drop_add_layernorm(one, one, None, 0.1, one, one, 1e-5, 4, 48, one, None) != 0 and b"regt_stae_add_layernorm:" in err()
    assert lib.regt_stae_drop_add_layernorm_backward_scratch_floats(4, 48) == 0
    assert lib.regt_stae_drop_add_layernorm_backward_scratch_floats(17, 32) == 2 * 2 * 32
    z = ctypes.c_void_p(512)
    assert lib.regt_stae_drop_add_layernorm_backward(one, one, one, -0.5, one, one, 1e-5, 4, 32, z, z, one, one, one, None) != 0 and b"[0, 1)" in err()
    assert lib.regt_stae_drop_add_layernorm_backward(one, one, one, 0.1, one, one, 1e-5, 4, 32, z, None, one, one, one, None) != 0 and b"NULL" in err()
    assert lib.regt_stae_drop_add_layernorm_backward(one, one, one, 0.1, one, one, 1e-5, 4, 32, z, z, one, one, one, None) != 0 and b"alias" in err()


def test_draw_stae_keep_shape_sites_packing_and_rate():
    torch.manual_seed(3)
    p, layers, rows, d = 0.1, 2, 500, 128
    keep = rnn.draw_stae_keep(layers, rows, d, "cpu", p)
    assert keep.dtype == torch.int32 and tuple(keep.shape) == (4 * layers, rows, d // 32)
    bits = unpack_keep(keep, d)
    n = bits.numel()
    assert abs(float(bits.double().mean()) - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5
    assert bool((keep < 0).any()), "bit 31 is never set: the words were not packed bytewise"
    per_bit = bits.reshape(-1, d // 32, 32).double().mean(dim=(0, 1))
    assert float((per_bit - (1 - p)).abs().max()) <= 5 * (p * (1 - p) / (n / 32)) ** 0.5          # every bit position is live
    assert torch.equal(pack_keep(bits), keep)
    # site order: one draw of (rows, D / 8, 8) uniforms per site, in site order, from the generator
    torch.manual_seed(3)
    for site in range(4 * layers):
        want = torch.rand(rows, d // 8, 8) >= p
        assert torch.equal(bits[site], want.reshape(rows, d)), site


def test_trainable_class_has_the_parents_parameters_and_the_parent_still_refuses():
    kw = dict(num_nodes=5, in_steps=3, out_steps=2, tod_embedding_dim=0, num_layers=1)
    torch.manual_seed(9)
    a = R.STAEformer(**kw)
    torch.manual_seed(9)
    b = R.STAEformerTrainable(**kw)
    assert "STAEformerTrainable" in R.__all__ and isinstance(b, R.STAEformer)
    assert list(a.state_dict()) == list(b.state_dict())
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    b.load_state_dict(a.state_dict(), strict=True)
    a.load_state_dict(b.state_dict(), strict=True)
    full = R.STAEformerTrainable(num_nodes=4, tod_embedding_dim=0)
    assert len(full.state_dict()) == 102 and full.last_keep is None
    with pytest.raises(R.RegtError):
        b(torch.zeros(1, 3, 5, 8))
    with pytest.raises(NotImplementedError):
        R.STAEformerTrainable(num_nodes=4)                       # model_dim 152: head width 38
    assert "STAEformer" not in R.train.MODELS and len(R.train.MODELS) == 11
    src = open(os.path.join(ROOT, "regt-gcn_amd", "nn.py")).read()
    assert "inference only" in src


def test_train_staeformer_parser():
    ap = train_staeformer.build_parser()
    a = ap.parse_args(["--fixture", "f.npz", "--num_timesteps_in", "6", "--num_timesteps_out", "1", "--tr", "0.5", "--tf", "occrate", "--snap_batch",
                       "4", "--epochs", "2", "--lr", "0.01", "--out_dir", "o"])
    assert (a.fixture, a.num_timesteps_in, a.num_timesteps_out, a.tr, a.tf, a.snap_batch, a.epochs, a.lr, a.out_dir) == \
        ("f.npz", 6, 1, 0.5, "occrate", 4, 2, 0.01, "o")
    ref = R.train.build_parser().parse_args([])
    d = ap.parse_args([])
    assert all(getattr(ref, k) == v for k, v in vars(d).items())               # train.py's own defaults
    for flag in ("--model", "--fused_step", "--decomp_type"):
        with pytest.raises(SystemExit):
            ap.parse_args([flag, "x"])


@pytest.mark.parametrize("name", sorted(TB.MODEL_CASES))
def test_gpu_cases_are_well_conditioned(name):
    case, (o64, g64), (o32, g32) = TB.model_case(name)
    ill, n = TB.ill_fraction(g32, g64, g32, case["dim"], case["scales"])
    print(f"{name}: {ill} of {n} blocks ill-conditioned")
    assert ill <= 0.05 * n
    TB.assert_blocks(g32, g64, g32, f"fp32 restatement, {name}", case["dim"], case["scales"])
    TB.forward_bar(o32, o64, o32, f"fp32 restatement forward, {name}")
    assert set(g64) == set(case["sd"])


@pytest.mark.parametrize("tag", TB.GOLDEN_RECORDS)
def test_float64_restatement_reproduces_the_reference_train_mode_records(tag):
    """The reference's unmodified module in train mode (r0: dropout 0; r1: dropout 0.1 under recorded keep words) against
    tests/staeformer_train_math.py: dropout placement, the 1 / (1 - p) scaling, the keep-word layout, run.py's loss and every recorded
    gradient.  No block of the golden is ill-conditioned."""
    case, (o_ref, l_ref, g_ref), (o64, l64, g64), (o32, l32, g32) = TB.golden_case(tag)
    TB.forward_bar(o_ref, o64, o32, f"golden {tag}: recorded out")
    TB.forward_bar(l_ref, l64, l32, f"golden {tag}: recorded losses")
    ill, n = TB.assert_blocks(g_ref, g64, g32, f"golden {tag}: recorded gradients", case["dim"], case["scales"], max_ill=0.0)
    assert not ill and TB.ill_fraction(g32, g64, g32, case["dim"], case["scales"])[0] == 0
    assert len(g_ref) == (38 if tag == "r1" else 26) and set(g_ref) <= set(case["sd"])
    if tag == "r1":
        bits = unpack_keep(case["keep"], case["dim"])
        assert tuple(case["keep"].shape) == (4, 2 * 6 * 33, 4) and abs(float(bits.double().mean()) - 0.9) <= 5 * (0.09 / bits.numel()) ** 0.5


def test_trainable_class_strict_loads_the_golden():
    case = TB.golden_case("r1")[0]
    mod = R.STAEformerTrainable(**case["kw"])
    assert list(mod.state_dict()) == list(case["sd"])
    mod.load_state_dict(case["sd"], strict=True)
    R.STAEformer(**case["kw"]).load_state_dict(case["sd"], strict=True)
