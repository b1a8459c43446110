"""grad_bars.assert_grads_to_scale on the CPU: the fp32 oracle passes it against the float64 oracle, and five corruptions of the
fp32 gradients -- each a wrong term of the kind a rewritten data- or weight-gradient kernel can produce -- fail it.  Next to
every corruption stands what the parity tests' own comparison (assert_allclose, atol = 1e-5, rtol = 1e-4, tensor by tensor)
says to it: that writes down which of them the old bar lets through.

Shape (777, 4000, 3, 8, 6, 3) with the parameters, inputs and loss of test_regt_matches_oracle_on_synthetic_regional_graph."""
import numpy as np
import pytest
import torch

from grad_bars import REL, assert_grads_to_scale, block_ratios, grad_blocks
from oracle import model as M
from test_gpu_grad_scale import _regt

N, E, REGIONS_, F, T, O = 777, 4000, 3, 8, 6, 3
NODE = 388                                             # the node whose loss term the last corruption removes
C = M.HIDDEN
RESET = "tgnn._base_tgcn.conv_r.lin.weight", "tgnn._base_tgcn.conv_r.bias", "tgnn._base_tgcn.linear_r.weight", "tgnn._base_tgcn.linear_r.bias"


def _mse(pred, hidden, y):
    return torch.mean((pred - y) ** 2)


def _mse_without_node(pred, hidden, y):
    keep = torch.ones(N, 1, dtype=pred.dtype)
    keep[NODE] = 0.0
    return torch.sum(keep * (pred - y) ** 2) / (N * O)


@pytest.fixture(scope="module")
def grads():
    case = _regt(N, E, REGIONS_, F, T, O)
    return {"f32": case.oracle_grads(torch.float32, _mse), "f64": case.oracle_grads(torch.float64, _mse),
            "f32_without_node": case.oracle_grads(torch.float32, _mse_without_node)}


def _old_bar_accepts(got, want):
    """The comparison of the parity tests: every tensor with assert_allclose(atol=1e-5, rtol=1e-4) against the fp32 oracle."""
    ok = True
    for k, w in want.items():
        if w is None:
            continue
        off = int((~np.isclose(got[k].numpy(), w.numpy(), atol=1e-5, rtol=1e-4)).sum())
        if off:
            print(f"  old bar: {k}: {off} of {w.numel()} elements off")
            ok = False
    return ok


def _zero_reset_gate(g, grads):
    for k in RESET:
        g[k] = torch.zeros_like(g[k])


def _scale_attention(g, grads):
    g["tgnn._attention"] = g["tgnn._attention"] * 1.1


def _scale_one_region_block(g, grads):
    g["tgnn.linear.weight"] = g["tgnn.linear.weight"].clone()
    g["tgnn.linear.weight"][:, C:2 * C] *= 1.01


def _negate_hidden_half_of_linear_r(g, grads):
    g["tgnn._base_tgcn.linear_r.weight"] = g["tgnn._base_tgcn.linear_r.weight"].clone()
    g["tgnn._base_tgcn.linear_r.weight"][:, C:] *= -1.0


def _drop_one_node_from_conv_r(g, grads):
    g["tgnn._base_tgcn.conv_r.lin.weight"] = grads["f32_without_node"]["tgnn._base_tgcn.conv_r.lin.weight"]


# (corruption, does the old atol = 1e-5 / rtol = 1e-4 comparison accept it?) -- the second column is what it DOES, recorded
CORRUPTIONS = [
    (_zero_reset_gate, False),                   # caught, but only by the handful of elements above 1e-5 (see the test below)
    (_scale_attention, True),
    (_scale_one_region_block, False),            # this tensor's scale is 5e-3: 1 % of it is above atol
    (_negate_hidden_half_of_linear_r, False),    # seen in the 2 % of the half's elements above 5e-6 only
    (_drop_one_node_from_conv_r, True),
]


def test_grad_blocks_split_what_separate_launches_produce():
    w = torch.arange(4 * 8, dtype=torch.float32).view(4, 8)
    for gate in "zrh":
        (l0, b0), (l1, b1) = grad_blocks(f"tgnn._base_tgcn.linear_{gate}.weight", w)
        assert torch.equal(b0, w[:, :4]) and torch.equal(b1, w[:, 4:]) and l0 != l1
    blocks = grad_blocks("tgnn.linear.weight", torch.zeros(4, 12), 3)
    assert [tuple(b.shape) for _l, b in blocks] == [(4, 4)] * 3
    assert len(grad_blocks("tgnn.linear.weight", torch.zeros(4, 12))) == 3          # region count from the shape
    for name, t in (("linear1.weight", torch.zeros(4, 8)), ("tgnn._base_tgcn.linear_z.bias", torch.zeros(4)), ("tgnn._attention", torch.zeros(6))):
        assert len(grad_blocks(name, t, 3)) == 1


def test_fp32_oracle_meets_the_bar_against_float64(grads):
    assert_grads_to_scale(grads["f32"], grads["f64"], REL, "fp32 oracle")
    rows = block_ratios(grads["f32"], grads["f64"])
    assert len(rows) == sum(1 for v in grads["f64"].values() if v is not None) + 3 + (REGIONS_ - 1)      # three halves, R blocks
    caps = {"default": 1e-4, "attention": 1e-3}                      # what REL may never exceed; the reference alone stays
    for _n, label, cls, err, scale in rows:                          # ~200x below (100x here: room for another summation order)
        print(f"  {label:60s} {cls:9s} scale {scale:.2e} fp32 oracle ratio {err / scale:.2e}")
        assert REL[cls] <= caps[cls] and err <= caps[cls] / 100 * scale, (label, err, scale)


@pytest.mark.parametrize("corrupt,old_bar_accepts", CORRUPTIONS, ids=[c.__name__.lstrip("_") for c, _ in CORRUPTIONS])
def test_corrupted_gradients_fail_the_bar(grads, corrupt, old_bar_accepts):
    g = dict(grads["f32"])
    corrupt(g, grads)
    with pytest.raises(AssertionError, match="off their own scale"):
        assert_grads_to_scale(g, grads["f64"], REL, corrupt.__name__)
    assert _old_bar_accepts(g, grads["f32"]) == old_bar_accepts


def test_old_bar_sees_a_zeroed_reset_gate_in_a_handful_of_elements_only(grads):
    """atol = 1e-5 rejects a reset gate that was never written only through the few elements above 1e-5: under 3 % of the
    weight gradients, under a quarter of the bias."""
    want = grads["f32"]
    for k, most in (("tgnn._base_tgcn.conv_r.lin.weight", 0.03), ("tgnn._base_tgcn.linear_r.weight", 0.03), ("tgnn._base_tgcn.conv_r.bias", 0.25)):
        seen = float((want[k].abs() > 1e-5 + 1e-4 * want[k].abs()).float().mean())
        print(f"  {k}: {seen:.4f} of the elements would show a zero gradient to the old bar")
        assert 0.0 < seen < most, (k, seen)


def test_exact_zero_rule_and_missing_gradients():
    want = {"a": torch.zeros(3, dtype=torch.float64), "b": None}
    assert_grads_to_scale({"a": torch.zeros(3), "b": None}, want, REL, "zeros")
    with pytest.raises(AssertionError):
        assert_grads_to_scale({"a": torch.tensor([0.0, 1e-30, 0.0]), "b": None}, want, REL, "nonzero where float64 is 0")
    with pytest.raises(AssertionError):
        assert_grads_to_scale({"a": torch.zeros(3), "b": torch.ones(2)}, want, REL, "a gradient where the oracle has none")
    with pytest.raises(AssertionError):
        assert_grads_to_scale({"a": None, "b": None}, want, REL, "no gradient where the oracle has one")
    with pytest.raises(AssertionError):
        assert_grads_to_scale({"a": torch.tensor([float("nan"), 0.0, 0.0]), "b": None}, {"a": torch.ones(3, dtype=torch.float64), "b": None}, REL, "nan")
