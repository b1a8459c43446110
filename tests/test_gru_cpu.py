"""StackedGRU without a GPU: the seeded rebuild of the goldens' parameters, the float64 restatement against the reference module's
goldens (training forward / backward, eval with the run.py / predict.py metrics, the three-window RMSprop trajectory) and against
torch.nn.GRU, the module's state_dict layout and seeded initialisation, the refusals, the command-line switches and the host-side
validation of the C entry points."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_npz
from gru_math import (GRAD_GAP, KEYS, LARGE, OUT_GAP, bar, build_params, check_stored, gru_layer, rel_err, rmsprop_first_step, sample,
                      stacked_gru, trajectory)

TAGS = ["in6_out1", "in12_out3"]


def _golden(tag):
    g = load_npz(f"golden_gru_{tag}.npz")
    return g, build_params(int(g["seed"]), int(g["t_in"]), int(g["t_out"]))


def _leaves(params):
    return {k: v.double().requires_grad_(True) for k, v in params.items()}


@pytest.mark.parametrize("tag", TAGS)
def test_rebuild_from_the_seed_matches_the_stored_samples_exactly(tag):
    g, params = _golden(tag)
    assert list(params) == KEYS and len(KEYS) == 12
    for k in KEYS:
        if k in LARGE:
            s, rs, cs = sample(params[k])
            np.testing.assert_array_equal(s.numpy(), g[f"p__{k}__s"])
            np.testing.assert_array_equal(rs.numpy(), g[f"p__{k}__rs"])
            np.testing.assert_array_equal(cs.numpy(), g[f"p__{k}__cs"])
        else:
            np.testing.assert_array_equal(params[k].numpy(), g[f"p__{k}"])
        assert torch.equal(params[k], params[k].to(torch.bfloat16).float())


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_training_golden(tag):
    g, params = _golden(tag)
    p = _leaves(params)
    out = stacked_gru(p, torch.from_numpy(g["x"]))
    loss = torch.mean((out[:, -1, :] - torch.from_numpy(g["y"]).double()) ** 2)
    loss.backward()
    assert rel_err(out, torch.from_numpy(g["train__out"])) <= bar(OUT_GAP[tag])
    assert abs(loss.item() - g["train__loss"][0]) <= bar(OUT_GAP[tag]) * g["train__loss"][0]
    check_stored(g, "train__g__", {k: p[k].grad for k in KEYS}, lambda k: bar(GRAD_GAP[tag][k]), "grad")


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_eval_golden_and_metrics(tag):
    g, params = _golden(tag)
    with torch.no_grad():
        out = stacked_gru({k: v.double() for k, v in params.items()}, torch.from_numpy(g["x"]))
    np.testing.assert_array_equal(g["eval__out"], g["train__out"])          # no dropout, no batch statistics
    assert rel_err(out, torch.from_numpy(g["eval__out"])) <= bar(OUT_GAP[tag])
    y = torch.from_numpy(g["y"]).double()
    err = (y - out[:, -1, :]).numpy()
    assert abs((err ** 2).mean() - g["eval__test_mse"][0]) <= 1e-6 * g["eval__test_mse"][0]
    assert abs(np.abs(err).mean() - g["eval__mae"][0]) <= 1e-6 * g["eval__mae"][0]
    assert abs((err ** 2).mean() - g["eval__mse"][0]) <= 1e-6 * g["eval__mse"][0]
    mape = (np.abs(err) / np.percentile(g["y"], q=95)).mean() * 100
    assert abs(mape - g["eval__mape"][0]) <= 1e-6 * g["eval__mape"][0]


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_trajectory(tag, tpims):
    g, params = _golden(tag)
    p = _leaves(params)
    w, t_in = int(g["window"]), int(g["t_in"])
    np.testing.assert_array_equal(g["x"], tpims["node_data"][:, :, w:w + t_in].numpy())
    losses = trajectory(tpims, g, lambda x, y: torch.mean((stacked_gru(p, x)[:, -1, :] - y.double()) ** 2))
    np.testing.assert_allclose(losses, g["traj__loss"], rtol=bar(OUT_GAP[tag]))
    steps, bounds = {}, {}
    for k in KEYS:
        # the fp32 reference's accumulated gradient is within its GRAD_GAP bar of this one; the step's sensitivity to it is lr eps / den^2,
        # and the fp32 parameter update itself rounds at 2^-24 of the parameter
        steps[k], sens = rmsprop_first_step(p[k].grad, p[k].detach())
        bounds[k] = sens * (bar(GRAD_GAP[tag][k]) * float(p[k].grad.abs().max())) + 2.0 ** -23 * p[k].detach().abs() + 32 * 2.0 ** -24 * 1e-2
    check_stored(g, "traj__dp__", steps, lambda k: bounds[k], "step")


@pytest.mark.parametrize("seq,rows,t,use_h0", [(1, 1, 1, False), (7, 3, 5, True), (20, 9, 12, True), (33, 2, 37, False)])
def test_restatement_equals_torch_gru_in_float64(seq, rows, t, use_h0):
    torch.manual_seed(seq * 100 + rows)
    ref = torch.nn.GRU(t, 256).double()
    x = torch.randn(seq, rows, t, dtype=torch.float64)
    h0 = torch.randn(1, rows, 256, dtype=torch.float64) if use_h0 else None
    dout, dlast = torch.randn(seq, rows, 256, dtype=torch.float64), torch.randn(1, rows, 256, dtype=torch.float64)
    o_r, l_r = ref(x, h0)
    ((o_r * dout).sum() + (l_r * dlast).sum()).backward()
    w = [q.detach().clone().requires_grad_(True) for q in ref.parameters()]
    o, l = gru_layer(x, *w, h0=h0)
    ((o * dout).sum() + (l * dlast[0]).sum()).backward()
    assert rel_err(o, o_r) < 1e-13 and rel_err(l, l_r[0]) < 1e-13
    for a, b in zip(w, ref.parameters()):
        assert rel_err(a.grad, b.grad) < 1e-12


@pytest.mark.parametrize("tag", TAGS)
def test_state_dict_layout_and_seeded_init_match_reference(tag):
    import regtgcn_amd as R
    g, params = _golden(tag)
    t_in, t_out = int(g["t_in"]), int(g["t_out"])
    torch.manual_seed(int(g["seed"]))
    mod = R.StackedGRU(t_in, 8, t_in, t_out)
    sd = mod.state_dict()
    assert list(sd.keys()) == KEYS and [k for k, _ in mod.named_parameters()] == KEYS
    assert tuple(sd["gru.weight_ih_l0"].shape) == (768, t_in) and tuple(sd["gru2.weight_hh_l0"].shape) == (768, 256)
    assert tuple(sd["linear2.weight"].shape) == (t_out, 256)
    for k in KEYS:                                                   # the goldens' parameters are this construction rounded to bf16
        assert torch.equal(sd[k].to(torch.bfloat16).float(), params[k]), k
    mod.load_state_dict(params, strict=True)


def test_constructor_signature_is_the_reference_one():
    import inspect
    import regtgcn_amd as R
    assert list(inspect.signature(R.StackedGRU.__init__).parameters) == ["self", "in_channels", "node_features", "periods", "output_dim"]
    assert list(inspect.signature(R.StackedGRU.forward).parameters)[:3] == ["self", "x", "edge_index"]


def test_refusals():
    import regtgcn_amd as R
    from regtgcn_amd import ops
    with pytest.raises(ValueError, match="input_size"):
        R.StackedGRU(0, 8, 0, 1)
    with pytest.raises(ValueError, match="input_size"):
        R.StackedGRU(256, 8, 256, 1)
    with pytest.raises(ValueError, match="output_dim"):
        R.StackedGRU(6, 8, 6, 0)
    with pytest.raises(ValueError, match="hidden"):
        ops.gru_limits(6, 128)
    mod = R.StackedGRU(6, 8, 6, 1)
    with pytest.raises(R.RegtError):
        mod(torch.zeros(10, 8, 6), None)                             # a CPU tensor
    with pytest.raises(R.RegtError):
        ops.gru_forward(torch.zeros(10, 8, 6), [q.detach() for q in mod.gru.parameters()])
    cpu = torch.device("cpu")
    w = [q.detach() for q in mod.gru.parameters()]
    ops.gru_check_weights(6, cpu, w)
    with pytest.raises(R.RegtError, match="on cuda:0"):               # module never moved to the GPU
        ops.gru_check_weights(6, torch.device("cuda:0"), w)
    noncontig = lambda t: torch.zeros(tuple(t.shape) + (2,))[..., 0]
    for bad in (lambda t: t.double(), lambda t: t.half(), noncontig, lambda t: t.reshape(-1, 1, *t.shape[1:])):
        for i in range(4):
            w2 = list(w)
            w2[i] = bad(w[i])
            with pytest.raises(R.RegtError):
                ops.gru_check_weights(6, cpu, w2)
    with pytest.raises(R.RegtError):
        ops.gru_check_weights(7, cpu, w)                              # another input size
    with pytest.raises(R.RegtError):
        ops.gru_check_weights(6, cpu, w[:3])
    small = torch.nn.GRU(6, 128)
    with pytest.raises(R.RegtError):                                  # a hidden size other than 256
        ops.gru_check_weights(6, cpu, [q.detach() for q in small.parameters()])


def test_parsers_accept_stacked_gru():
    import regtgcn_amd as R
    a = R.train.build_parser().parse_args(["--model", "StackedGRU", "--snap_batch", "64"])
    assert a.model == "StackedGRU" and a.snap_batch == 64
    assert "StackedGRU" in R.train.MODELS
    b = R.evaluate.build_parser().parse_args(["--model", "StackedGRU", "--checkpoint", "c.pt"])
    assert b.model == "StackedGRU"


def test_gru_entry_points_validate_on_the_host():
    """Bad dims and NULL pointers are refused with a message that names the field before anything touches a GPU."""
    from regtgcn_amd import _lib
    import regtgcn_amd as R
    lib = R.load_library()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)
    p += -p % 16

    def dims(**kw):
        d = dict(seq_len=104, rows=8, input_size=12, hidden=256, training=1, x_stride_seq=96, x_stride_row=12, x_stride_t=1)
        d.update(kw)
        return _lib.GruDims(*d.values())

    ws, sc = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.regt_gru_sizes(ctypes.byref(dims()), ctypes.byref(ws), ctypes.byref(sc)) == 0
    packed = 256 * 768 + 12 * 768
    assert ws.value == packed + (104 + 1) * 8 * 256 + 104 * 8 * 4 * 256 and sc.value > 104 * 8 * 1024
    assert lib.regt_gru_sizes(ctypes.byref(dims(training=0)), ctypes.byref(ws), ctypes.byref(sc)) == 0
    assert ws.value == packed
    for bad, word in ((dict(hidden=128), b"hidden"), (dict(hidden=512), b"hidden"), (dict(input_size=0), b"input_size"),
                      (dict(input_size=256), b"input_size"), (dict(seq_len=0), b"seq_len"), (dict(rows=0), b"rows"),
                      (dict(seq_len=1 << 20, rows=1 << 12), b"seq_len * rows"), (dict(x_stride_row=-1), b"strides")):
        assert lib.regt_gru_sizes(ctypes.byref(dims(**bad)), ctypes.byref(ws), ctypes.byref(sc)) != 0, bad
        assert word in lib.regt_last_error(), (bad, lib.regt_last_error())
    d = ctypes.byref(dims())
    null_table = (ctypes.c_void_p * 4)()
    full = (ctypes.c_void_p * 4)(*([p] * 4))
    assert lib.regt_gru_forward(d, None, p, p, p, p, None, p, p, p, None) != 0
    assert b"NULL" in lib.regt_last_error()
    assert lib.regt_gru_forward(d, p, p, None, p, p, None, p, p, p, None) != 0
    assert b"weight" in lib.regt_last_error()
    assert lib.regt_gru_forward(d, p, p, p, p, p, None, p, p, None, None) != 0
    assert b"workspace" in lib.regt_last_error()
    assert lib.regt_gru_forward(d, p, p, p, p, p, None, None, None, p, None) != 0
    assert b"out and h_last" in lib.regt_last_error()
    assert lib.regt_gru_forward(ctypes.byref(dims(hidden=64)), p, p, p, p, p, None, p, p, p, None) != 0
    assert b"hidden" in lib.regt_last_error()
    assert lib.regt_gru_backward(d, p, null_table, None, p, None, full, None, p, p, None) != 0
    assert b"weights" in lib.regt_last_error() and b"NULL" in lib.regt_last_error()
    assert lib.regt_gru_backward(d, p, full, None, p, None, None, None, p, p, None) != 0
    assert b"grads" in lib.regt_last_error()
    assert lib.regt_gru_backward(d, p, full, None, None, None, full, None, p, p, None) != 0
    assert b"dout and dh_last" in lib.regt_last_error()
    assert lib.regt_gru_backward(d, p, full, None, p, None, full, None, None, p, None) != 0
    assert b"workspace" in lib.regt_last_error()
    assert lib.regt_gru_backward(ctypes.byref(dims(training=0)), p, full, None, p, None, full, None, p, p, None) != 0
    assert b"training" in lib.regt_last_error()
    assert lib.regt_gru_backward(ctypes.byref(dims(input_size=300)), p, full, None, p, None, full, None, p, p, None) != 0
    assert b"input_size" in lib.regt_last_error()
    assert lib.regt_relu_backward(None, p, 4, None) != 0 and b"NULL" in lib.regt_last_error()
    assert lib.regt_relu_backward(p, p, 0, None) != 0 and b"n must be" in lib.regt_last_error()
    assert lib.regt_relu_backward(p, p, 1 << 31, None) != 0 and b"n must be" in lib.regt_last_error()
