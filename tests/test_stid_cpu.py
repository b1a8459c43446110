"""STID without a GPU: the float64 restatement against the reference module's goldens (training forward / backward with the keep
mask the reference drew, eval with the run.py / predict.py metrics, the three-window trajectory's losses), the module's state_dict
layout and seeded initialisation, the refusals, the command-line switches and the host-side validation of the C entry points."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_npz
from stid_math import pack_keep, stid, unpack_keep

TAGS = ["in6_out1", "in12_out3"]
# the largest gap between stid_math in float64 and the reference module's recorded fp32 gradients (one thread), as
# tools/make_stid_goldens.py printed it when it wrote the files: 6.14e-8 (in6_out1), 3.34e-8 (in12_out3); outputs 1.4e-7
GRAD_GAP = 7e-8


def _golden(tag):
    g = load_npz(f"golden_stid_{tag}.npz")
    keys = [str(k) for k in g["state_dict_keys"]]
    return g, keys, {k: torch.from_numpy(g[f"p__{k}"]) for k in keys}


def _leaves(params):
    return {k: v.double().requires_grad_(True) for k, v in params.items()}


def test_keep_bit_layout_round_trips():
    keep = torch.rand(2, 1, 5, 64, generator=torch.Generator().manual_seed(0)) < 0.85
    keep[0, 0, 0, 31] = keep[0, 0, 0, 63] = True
    words = pack_keep(keep)
    assert words.dtype == torch.int32 and tuple(words.shape) == (2, 1, 5, 2)
    assert torch.equal(unpack_keep(words), keep)
    assert int(words[0, 0, 0, 0]) < 0 and int(words[0, 0, 0, 1]) < 0          # channel 31 / 63 is the word's top bit
    assert bool((int(words[1, 0, 2, 1]) >> 3) & 1) == bool(keep[1, 0, 2, 35])


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_training_golden(tag):
    g, keys, params = _golden(tag)
    assert len(keys) == 17
    p = _leaves(params)
    keep = unpack_keep(torch.from_numpy(g["train__keep"]))
    assert tuple(keep.shape) == (3, 1, 104, 64)
    out = stid(p, torch.from_numpy(g["x"]), 3, keep=keep)
    loss = torch.mean((out - torch.from_numpy(g["y"]).double()) ** 2)
    loss.backward()
    np.testing.assert_allclose(out.detach().numpy(), g["train__out"], atol=1e-5)
    assert abs(loss.item() - g["train__loss"][0]) < 1e-5
    for k in keys:
        assert float(np.abs(p[k].grad.numpy() - g[f"train__g__{k}"]).max()) < 1e-5 + GRAD_GAP, k


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_eval_golden_and_metrics(tag):
    g, keys, params = _golden(tag)
    with torch.no_grad():
        out = stid(params, torch.from_numpy(g["x"]), 3)
    y = torch.from_numpy(g["y"]).double()
    np.testing.assert_allclose(out.numpy(), g["eval__out"], atol=1e-5)
    assert abs(((out[0][0] - y) ** 2).mean().item() - g["eval__test_mse"][0]) < 1e-5
    err = (y - out).numpy()
    assert abs(np.abs(err).mean() - g["eval__mae"][0]) < 1e-5
    assert abs((err ** 2).mean() - g["eval__mse"][0]) < 1e-5
    assert abs(np.abs(err).mean() / np.percentile(y.numpy(), q=95) * 100 - g["eval__mape"][0]) < 1e-3


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_trajectory_losses(tag, tpims):
    g, keys, params = _golden(tag)
    p = _leaves(params)
    t_in, t_out, w = int(g["t_in"]), int(g["t_out"]), int(g["window"])
    np.testing.assert_array_equal(g["x"][0], tpims["node_data"][:, :, w:w + t_in].permute(2, 0, 1).numpy())
    losses = []
    for k in range(3):
        x = tpims["node_data"][:, :, w + k:w + k + t_in].permute(2, 0, 1).unsqueeze(0)
        y = tpims["node_data"][:, -1, w + k + t_in:w + k + t_in + t_out].double()
        out = stid(p, x, 3, keep=unpack_keep(torch.from_numpy(g["traj__keep"][k])))
        loss = torch.mean((out - y) ** 2)
        loss.backward()
        losses.append(loss.item())
    np.testing.assert_allclose(losses, g["traj__loss"], atol=1e-5)


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_layout_and_seeded_init_match_reference(tag):
    import regtgcn_amd as R
    g, keys, params = _golden(tag)
    torch.manual_seed(int(g["seed"]))
    mod = R.STID(num_nodes=104, input_len=int(g["t_in"]), output_len=int(g["t_out"]), if_time_in_day=False, if_day_in_week=False)
    sd = mod.state_dict()
    assert list(sd.keys()) == keys and len(keys) == 17
    for k, v in params.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    assert sd["encoder.0.fc1.weight"].dim() == 4 and sd["regression_layer.weight"].dim() == 4
    assert [k for k, _ in mod.named_parameters()] == keys
    np.testing.assert_array_equal(sd["node_emb"].numpy(), g["init__node_emb"])
    np.testing.assert_array_equal(sd["time_series_emb_layer.weight"].numpy(), g["init__time_series_emb_layer.weight"])
    mod.load_state_dict(params, strict=True)


def test_constructor_signature_is_the_reference_one():
    import inspect
    import regtgcn_amd as R
    sig = inspect.signature(R.STID.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [
        ("input_len", 12), ("output_len", 12), ("input_dim", 3), ("embed_dim", 32), ("node_dim", 32), ("temp_dim_tid", 32),
        ("temp_dim_diw", 32), ("time_of_day_size", 288), ("day_of_week_size", 7), ("if_node", True), ("if_time_in_day", True),
        ("if_day_in_week", True), ("num_layer", 3)]
    assert list(sig.parameters)[1] == "num_nodes"


def test_constructor_refusals_and_cpu_input():
    import regtgcn_amd as R
    off = dict(if_time_in_day=False, if_day_in_week=False)
    with pytest.raises(ValueError, match="if_time_in_day"):
        R.STID(10)                                                # the reference's defaults switch the temporal embeddings on
    with pytest.raises(ValueError, match="if_time_in_day"):
        R.STID(10, if_time_in_day=False)
    with pytest.raises(ValueError, match="if_time_in_day"):
        R.STID(10, if_day_in_week=False)
    with pytest.raises(ValueError, match="embed_dim"):
        R.STID(10, embed_dim=16, **off)
    with pytest.raises(ValueError, match="num_layer"):
        R.STID(10, num_layer=9, **off)
    with pytest.raises(ValueError, match="output_len"):
        R.STID(10, output_len=0, **off)
    with pytest.raises(ValueError, match="input_len"):
        R.STID(10, input_len=25, input_dim=8, **off)
    R.STID(10, input_len=24, input_dim=8, **off)
    mod = R.STID(10, input_len=6, output_len=1, **off)
    assert mod.hidden_dim == 64 and R.STID(10, if_node=False, **off).hidden_dim == 32
    with pytest.raises(R.RegtError):
        mod(torch.zeros(1, 6, 10, 8))


def test_tensor_tables_are_checked_before_any_launch():
    """The kernels read the parameters through raw pointers: a module left on the host, another dtype, a non-contiguous tensor or a
    wrong shape is refused on the host -- here against a CUDA device that is never touched."""
    import regtgcn_amd as R
    from regtgcn_amd import ops
    mod = R.STID(10, input_len=6, output_len=2, if_time_in_day=False, if_day_in_week=False)
    dims = ops.stid_dims(10, 2, 6, 8, 3, 3, 2)
    with pytest.raises(R.RegtError, match="on cuda:0"):                 # module never moved to the GPU
        ops.stid_check_tables(dims, torch.device("cuda:0"), mod.param_table())
    cpu = torch.device("cpu")
    params = mod.param_table()
    assert len(params) == 17
    ops.stid_check_tables(dims, cpu, params)                              # the same table on its own device passes
    noncontig = lambda t: torch.zeros(tuple(t.shape) + (2,))[..., 0]      # same shape and dtype, strided
    for bad in (lambda t: t.double(), lambda t: t.half(), noncontig, lambda t: t.reshape(-1, 1)):
        for i in (0, 1, 5, 15):
            p2 = list(params)
            p2[i] = bad(params[i].detach())
            with pytest.raises(R.RegtError):
                ops.stid_check_tables(dims, cpu, p2)
    with pytest.raises(R.RegtError):                                     # a node embedding where the dims say if_node is off
        ops.stid_check_tables(ops.stid_dims(10, 2, 6, 8, 3, 3, 2, if_node=False), cpu, params)
    with pytest.raises(R.RegtError):
        ops.stid_check_tables(dims, cpu, params[:-1])
    with pytest.raises(R.RegtError):                                     # another output_len
        ops.stid_check_tables(ops.stid_dims(10, 2, 6, 8, 3, 3, 4), cpu, params)


def test_parsers_accept_stid():
    import regtgcn_amd as R
    a = R.train.build_parser().parse_args(["--model", "STID", "--snap_batch", "16"])
    assert a.model == "STID" and a.snap_batch == 16
    assert "STID" in R.train.MODELS
    b = R.evaluate.build_parser().parse_args(["--model", "STID", "--checkpoint", "c.pt"])
    assert b.model == "STID"


def test_stid_entry_points_validate_on_the_host():
    """Bad dims and NULL tables are refused with a message that names the field before anything touches a GPU."""
    from regtgcn_amd import _lib
    import regtgcn_amd as R
    lib = R.load_library()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)

    def dims(**kw):
        d = dict(num_nodes=104, batch=1, input_len=6, in_features=8, input_dim=3, embed_dim=32, node_dim=32, num_layer=3, output_len=1,
                 if_node=1, dropout_p=0.15)
        d.update(kw)
        return _lib.StidDims(*d.values())

    ws, sc = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.regt_stid_sizes(ctypes.byref(dims()), ctypes.byref(ws), ctypes.byref(sc)) == 0
    assert ws.value == 7 * 104 * 64 and sc.value > 0
    assert lib.regt_stid_sizes(ctypes.byref(dims(input_dim=8, input_len=24, if_node=0, num_layer=8, output_len=64)), ctypes.byref(ws),
                               ctypes.byref(sc)) == 0
    for bad, word in ((dict(num_nodes=0), b"num_nodes"), (dict(batch=0), b"batch"), (dict(input_len=0), b"input_len"),
                      (dict(input_len=256), b"input_len"), (dict(input_dim=0), b"input_dim"), (dict(input_dim=9), b"input_dim"),
                      (dict(in_features=257, input_dim=1), b"in_features"), (dict(input_dim=8, input_len=25), b"input_dim * input_len"),
                      (dict(embed_dim=16), b"embed_dim"), (dict(node_dim=64), b"node_dim"), (dict(num_layer=0), b"num_layer"),
                      (dict(num_layer=9), b"num_layer"), (dict(output_len=0), b"output_len"), (dict(output_len=65), b"output_len"),
                      (dict(dropout_p=1.0), b"dropout_p")):
        assert lib.regt_stid_sizes(ctypes.byref(dims(**bad)), ctypes.byref(ws), ctypes.byref(sc)) != 0, bad
        assert word in lib.regt_last_error(), (bad, lib.regt_last_error())
    null_table = (ctypes.c_void_p * 64)()
    full = (ctypes.c_void_p * 64)(*([p] * 64))
    d = ctypes.byref(dims())
    assert lib.regt_stid_forward(d, p, null_table, None, p, p, None) != 0
    assert b"node_emb" in lib.regt_last_error() and b"NULL" in lib.regt_last_error()
    assert lib.regt_stid_forward(d, p, None, None, p, p, None) != 0
    assert b"NULL" in lib.regt_last_error()
    assert lib.regt_stid_forward(d, None, full, None, p, p, None) != 0
    assert b"NULL" in lib.regt_last_error()
    assert lib.regt_stid_forward(ctypes.byref(dims(num_layer=9)), p, full, None, p, p, None) != 0
    assert b"num_layer" in lib.regt_last_error()
    assert lib.regt_stid_backward(d, p, full, None, p, null_table, p, p, None) != 0
    assert b"grads" in lib.regt_last_error() and b"NULL" in lib.regt_last_error()
    assert lib.regt_stid_backward(d, p, full, None, p, full, None, p, None) != 0
    assert b"workspace" in lib.regt_last_error()
    assert lib.regt_stid_backward(ctypes.byref(dims(output_len=0)), p, full, None, p, full, p, p, None) != 0
    assert b"output_len" in lib.regt_last_error()
