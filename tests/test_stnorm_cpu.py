"""STNorm without a GPU: the float64 restatement against the reference module's goldens (training forward / backward with the
running buffers, eval with the updated buffers and the run.py / predict.py metrics, the three-snapshot trajectory's losses), the
module's state_dict layout, the command-line switches and the host-side validation of the new C entry points."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_npz
from stnorm_math import stnorm

TAGS = ["in6_out1", "in12_out3"]
GRAD_GAP = 4e-6          # the bound tests/test_gpu_stnorm.py uses for the fp32-vs-float64 gradient gap


def _golden(tag):
    g = load_npz(f"golden_stnorm_{tag}.npz")
    keys = [str(k) for k in g["state_dict_keys"]]
    return g, keys, {k: torch.from_numpy(g[f"p__{k}"]) for k in keys}


def _leaves(params):
    p = {k: v.double() for k, v in params.items()}
    for k in p:
        if "running" not in k:
            p[k].requires_grad_(True)
    return p


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_training_golden(tag):
    g, keys, params = _golden(tag)
    p = _leaves(params)
    out, bufs = stnorm(p, torch.from_numpy(g["x"]))
    loss = torch.mean((out - torch.from_numpy(g["y"]).double()) ** 2)
    loss.backward()
    np.testing.assert_allclose(out.detach().numpy(), g["train__out"], atol=1e-5)
    assert abs(loss.item() - g["train__loss"][0]) < 1e-5
    gnone = {str(k) for k in g["train__gnone"]}
    assert gnone == {"residual_convs.7.weight", "residual_convs.7.bias"}
    worst = 0.0
    for k in keys:
        if "running" in k:
            continue
        if k in gnone:
            assert p[k].grad is None
            continue
        worst = max(worst, float(np.abs(p[k].grad.numpy() - g[f"train__g__{k}"]).max()))
    assert worst < GRAD_GAP
    for k, v in bufs.items():
        np.testing.assert_allclose(v.numpy(), g[f"train__b__{k}"], atol=1e-6)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_eval_golden_and_metrics(tag):
    g, keys, params = _golden(tag)
    p = {k: (torch.from_numpy(g[f"train__b__{k}"]) if "running" in k else v) for k, v in params.items()}
    with torch.no_grad():
        out, _ = stnorm(p, torch.from_numpy(g["x"]), training=False)
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
    t_in, t_out, w, n = int(g["t_in"]), int(g["t_out"]), int(g["window"]), int(g["nodes"])
    np.testing.assert_array_equal(g["x"][0], tpims["node_data"][:n, :, w:w + t_in].permute(2, 0, 1).numpy())
    losses = []
    for k in range(3):
        x = tpims["node_data"][:n, :, w + k:w + k + t_in].permute(2, 0, 1).unsqueeze(0)
        y = tpims["node_data"][:n, -1, w + k + t_in:w + k + t_in + t_out].double()
        out, bufs = stnorm(p, x)
        loss = torch.mean((out - y) ** 2)
        loss.backward()
        losses.append(loss.item())
        p.update(bufs)
    np.testing.assert_allclose(losses, g["traj__loss"], atol=1e-5)
    for k, v in bufs.items():
        np.testing.assert_allclose(v.numpy(), g[f"traj__b__{k}"], atol=1e-6)


def test_tnorm_group_one_equals_sequential_snapshots():
    g, keys, params = _golden("in6_out1")
    x = torch.from_numpy(g["x"]).double()
    xb = torch.cat([x, x.flip(2)], 0)
    with torch.no_grad():
        ob, bb = stnorm(params, xb, tnorm_group=1)
        o0, b0 = stnorm(params, xb[:1])
        p1 = {**params, **b0}
        o1, b1 = stnorm(p1, xb[1:])
    np.testing.assert_allclose(ob.numpy(), torch.cat([o0, o1]).numpy(), atol=1e-12)
    for k in bb:
        np.testing.assert_allclose(bb[k].numpy(), b1[k].numpy(), atol=1e-12)


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_layout_matches_reference(tag):
    import regtgcn_amd as R
    g, keys, params = _golden(tag)
    mod = R.STNorm(num_nodes=g["x"].shape[2], in_dim=8, out_dim=int(g["t_out"]))
    sd = mod.state_dict()
    assert list(sd.keys()) == keys and len(keys) == 118
    for k, v in params.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
    mod.load_state_dict(params, strict=True)


def test_module_refuses_cpu_and_unsupported_shapes():
    import regtgcn_amd as R
    with pytest.raises(ValueError):
        R.STNorm(10, channels=32)
    with pytest.raises(ValueError):
        R.STNorm(10, kernel_size=3)
    mod = R.STNorm(10, in_dim=2, out_dim=1)
    with pytest.raises(R.RegtError):
        mod(torch.zeros(1, 6, 10, 2))


def test_module_refuses_out_of_range_dims_at_construction():
    import regtgcn_amd as R
    with pytest.raises(ValueError):
        R.STNorm(10, in_dim=257)
    with pytest.raises(ValueError):
        R.STNorm(10, out_dim=0)


def test_tensor_tables_are_checked_before_any_launch():
    """The kernels read parameters and buffers through raw pointers: a module left on the host, another dtype, a non-contiguous
    tensor or a wrong shape is refused on the host -- here against a CUDA device that is never touched."""
    import regtgcn_amd as R
    from regtgcn_amd import ops
    mod = R.STNorm(10, in_dim=3, out_dim=2)
    dims = ops.stnorm_dims(10, 2, 2, 6, 3, 2, mod.blocks, mod.layers, True, True, True)
    cuda = torch.device("cuda:0")
    with pytest.raises(R.RegtError, match="on cuda:0"):                 # module never moved to the GPU
        ops.stnorm_check_tables(dims, cuda, mod.param_table(), mod.running_table())
    cpu = torch.device("cpu")
    ops.stnorm_check_tables(dims, cpu, mod.param_table(), mod.running_table())     # the same tables on their own device pass
    params, running = mod.param_table(), mod.running_table()
    noncontig = lambda t: torch.zeros(tuple(t.shape) + (2,))[..., 0]      # same shape and dtype, strided
    for bad in (lambda t: t.double(), lambda t: t.half(), noncontig, lambda t: t.reshape(-1)):
        p2 = list(params)
        p2[0] = bad(params[0].detach())
        with pytest.raises(R.RegtError):
            ops.stnorm_check_tables(dims, cpu, p2, running)
        r2 = list(running)
        r2[3] = bad(running[3])
        with pytest.raises(R.RegtError):
            ops.stnorm_check_tables(dims, cpu, params, r2)
    with pytest.raises(R.RegtError):                                     # a SNorm entry where the dims say SNorm is off
        ops.stnorm_check_tables(ops.stnorm_dims(10, 2, 2, 6, 3, 2, mod.blocks, mod.layers, True, False, True), cpu, params, running)
    with pytest.raises(R.RegtError):
        ops.stnorm_check_tables(dims, cpu, params, running[:-1])


def test_parsers_accept_stnorm():
    import regtgcn_amd as R
    a = R.train.build_parser().parse_args(["--model", "STNorm", "--snap_batch", "16"])
    assert a.model == "STNorm" and a.snap_batch == 16
    assert "STNorm" in R.train.MODELS
    b = R.evaluate.build_parser().parse_args(["--model", "STNorm", "--checkpoint", "c.pt"])
    assert b.model == "STNorm"


def test_stnorm_entry_points_validate_on_the_host():
    """Bad dims and NULL tables are refused with a message before anything touches a GPU."""
    from regtgcn_amd import _lib
    import regtgcn_amd as R
    lib = R.load_library()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)

    def dims(**kw):
        d = dict(num_nodes=104, batch=1, tnorm_group=1, seq_len=6, in_dim=8, out_dim=1, blocks=4, layers=2, tnorm=1, snorm=1,
                 training=1)
        d.update(kw)
        return _lib.StnormDims(*d.values())

    ws, sc = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.regt_stnorm_sizes(ctypes.byref(dims()), ctypes.byref(ws), ctypes.byref(sc)) == 0
    assert ws.value > 0 and sc.value > 0
    for bad, word in ((dict(num_nodes=1), b"num_nodes"), (dict(tnorm_group=3, batch=4), b"tnorm_group"), (dict(seq_len=0), b"seq_len"),
                      (dict(in_dim=0), b"in_dim"), (dict(out_dim=300), b"out_dim"), (dict(layers=9), b"layers"),
                      (dict(blocks=0), b"blocks")):
        assert lib.regt_stnorm_sizes(ctypes.byref(dims(**bad)), ctypes.byref(ws), ctypes.byref(sc)) != 0, bad
        assert word in lib.regt_last_error(), bad
    null_table = (ctypes.c_void_p * 200)()
    full = (ctypes.c_void_p * 200)(*([p] * 200))
    d = ctypes.byref(dims())
    assert lib.regt_stnorm_forward(d, p, null_table, full, p, p, None) != 0
    assert b"NULL" in lib.regt_last_error()
    assert lib.regt_stnorm_forward(d, p, full, None, p, p, None) != 0
    assert b"running" in lib.regt_last_error()
    assert lib.regt_stnorm_forward(d, None, full, full, p, p, None) != 0
    assert lib.regt_stnorm_backward(d, p, full, full, p, null_table, p, p, None) != 0
    assert b"NULL" in lib.regt_last_error()
    assert lib.regt_stnorm_backward(ctypes.byref(dims(num_nodes=1)), p, full, full, p, full, p, p, None) != 0
