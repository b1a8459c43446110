"""The Python bridge without a GPU: gradient delivery under set_grad_accumulation_in_backward, the context manager that switches it
on, the cell's parameter list, and the one table checker behind stnorm_check_tables, stid_check_tables and gru_check_weights."""
import re

import pytest
import torch


@pytest.fixture
def F():
    import regtgcn_amd as R
    prev = R.functional.set_grad_accumulation_in_backward(False)
    yield R.functional
    R.functional.set_grad_accumulation_in_backward(prev)


def _leaves(gen, with_grad):
    """Five leaf parameters (entry 1 of the table is None), their gradients (entry 3 is None) and the ``.grad`` two of them hold."""
    shapes = [(3, 4), None, (5,), (2, 2), (7, 1)]
    params = [None if s is None else torch.randn(*s, generator=gen).requires_grad_(True) for s in shapes]
    grads = [None if s is None else torch.randn(*s, generator=gen) for s in shapes]
    grads[3] = None
    old = {}
    for i in with_grad:
        params[i].grad = torch.randn(*shapes[i], generator=gen)
        old[i] = params[i].grad.clone()
    return params, grads, old


def test_deliver_grads_returns_them_with_the_switch_off(F):
    params, grads, old = _leaves(torch.Generator().manual_seed(1), with_grad=(2,))
    out = F._deliver_grads(params, grads)
    assert isinstance(out, tuple) and len(out) == len(params)
    assert all(a is b for a, b in zip(out, grads))                          # as given, None entries kept
    assert params[0].grad is None and params[4].grad is None and torch.equal(params[2].grad, old[2])


def test_deliver_grads_accumulates_with_the_switch_on(F):
    F.set_grad_accumulation_in_backward(True)
    params, grads, old = _leaves(torch.Generator().manual_seed(2), with_grad=(2, 4))
    held = {i: params[i].grad for i in old}
    out = F._deliver_grads(params, grads)
    assert out == (None,) * len(params)
    assert params[0].grad is grads[0]                                       # no .grad before: the gradient tensor itself
    for i in old:                                                           # .grad before: added in place, bit for bit old + g
        assert params[i].grad is held[i] and torch.equal(params[i].grad, old[i] + grads[i])
    assert params[3].grad is None                                           # (p, None) is skipped; (None, None) is entry 1
    # a second delivery adds to what the first one left, the tensor handed over included
    g2 = [None if g is None else torch.full_like(g, 0.5) for g in grads]
    want = {i: params[i].grad.clone() + g2[i] for i in (0, 2, 4)}
    assert F._deliver_grads(params, g2) == (None,) * len(params)
    assert all(torch.equal(params[i].grad, want[i]) for i in want) and params[0].grad is grads[0]


@pytest.mark.parametrize("spoil", ["non_leaf", "frozen"])
def test_deliver_grads_leaves_foreign_tensors_to_autograd(F, spoil):
    F.set_grad_accumulation_in_backward(True)
    params, grads, old = _leaves(torch.Generator().manual_seed(3), with_grad=(2,))
    params[4] = params[4] * 2.0 if spoil == "non_leaf" else params[4].detach()
    assert (not params[4].is_leaf) if spoil == "non_leaf" else (not params[4].requires_grad)
    out = F._deliver_grads(params, grads)
    assert len(out) == len(params) and all(a is b for a, b in zip(out, grads))
    assert params[0].grad is None and torch.equal(params[2].grad, old[2])   # nothing was accumulated


def test_context_manager_restores_and_nests(F):
    assert F._ACCUMULATE_IN_BACKWARD is False
    with F.grad_accumulation_in_backward():
        assert F._ACCUMULATE_IN_BACKWARD is True
        with F.grad_accumulation_in_backward():
            assert F._ACCUMULATE_IN_BACKWARD is True
        assert F._ACCUMULATE_IN_BACKWARD is True                            # the inner exit restores the outer setting, not the default
    assert F._ACCUMULATE_IN_BACKWARD is False
    with pytest.raises(KeyError):
        with F.grad_accumulation_in_backward():
            raise KeyError("body")
    assert F._ACCUMULATE_IN_BACKWARD is False
    assert F.set_grad_accumulation_in_backward(True) is False               # the setter still returns the previous setting
    with pytest.raises(KeyError):
        with F.grad_accumulation_in_backward():
            raise KeyError("body")
    assert F._ACCUMULATE_IN_BACKWARD is True                                # on before, on after


def test_param_names_cell_is_the_list_it_was(F):
    assert F.PARAM_NAMES_CELL == [
        "tgnn._attention",
        "tgnn._base_tgcn.conv_z.lin.weight", "tgnn._base_tgcn.conv_r.lin.weight", "tgnn._base_tgcn.conv_h.lin.weight",
        "tgnn._base_tgcn.conv_z.bias", "tgnn._base_tgcn.conv_r.bias", "tgnn._base_tgcn.conv_h.bias",
        "tgnn._base_tgcn.linear_z.weight", "tgnn._base_tgcn.linear_r.weight", "tgnn._base_tgcn.linear_h.weight",
        "tgnn._base_tgcn.linear_z.bias", "tgnn._base_tgcn.linear_r.bias", "tgnn._base_tgcn.linear_h.bias",
        "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"]
    assert F.param_names(False) == F.PARAM_NAMES_COMMON + F.PARAM_NAMES_HEAD and len(F.param_names(True)) == 22


def _stnorm_case():
    import regtgcn_amd as R
    from regtgcn_amd import ops
    mod = R.STNorm(10, in_dim=3, out_dim=2)
    dims = lambda snorm=True: ops.stnorm_dims(10, 2, 2, 6, 3, 2, mod.blocks, mod.layers, True, snorm, True)
    running = mod.running_table()
    check = lambda table, snorm=True: ops.stnorm_check_tables(dims(snorm), torch.device("cpu"), table, running, "lbl")
    off = R.STNorm(10, snorm_bool=False, in_dim=3, out_dim=2).param_table()
    # entry 6: the first layer's filter conv; entry 16: its first SNorm parameter, None when SNorm is off
    return check, [p.detach() for p in mod.param_table()], "parameter", 6, (lambda t: check(t, False), off, 16, "TNorm / SNorm off")


def _stnorm_running_case():
    import regtgcn_amd as R
    from regtgcn_amd import ops
    mod = R.STNorm(10, in_dim=3, out_dim=2)
    dims = ops.stnorm_dims(10, 2, 2, 6, 3, 2, mod.blocks, mod.layers, True, True, True)
    params = mod.param_table()
    check = lambda table: ops.stnorm_check_tables(dims, torch.device("cpu"), params, table, "lbl")
    return check, list(mod.running_table()), "running buffer", 3, None


def _stid_case():
    import regtgcn_amd as R
    from regtgcn_amd import ops
    mod = R.STID(10, input_len=6, output_len=2, if_time_in_day=False, if_day_in_week=False)
    dims = lambda if_node=True: ops.stid_dims(10, 2, 6, 8, 3, 3, 2, if_node=if_node)
    check = lambda table, if_node=True: ops.stid_check_tables(dims(if_node), torch.device("cpu"), table, "lbl")
    off = R.STID(10, input_len=6, output_len=2, if_node=False, if_time_in_day=False, if_day_in_week=False).param_table()
    return check, [p.detach() for p in mod.param_table()], "parameter", 5, (lambda t: check(t, False), off, 0, "if_node off")


def _gru_case():
    from regtgcn_amd import ops
    weights = [q.detach() for q in torch.nn.GRU(6, 256).parameters()]
    return (lambda table: ops.gru_check_weights(6, torch.device("cpu"), table, "lbl")), weights, "weight", 1, None


@pytest.mark.parametrize("case", [_stnorm_case, _stnorm_running_case, _stid_case, _gru_case])
def test_table_checker_names_the_entry_and_its_shape(case):
    """The same bad entry gets the same refusal through each public function: RegtError naming the label, the kind of entry, its
    index and the shape it must have."""
    import regtgcn_amd as R
    check, table, kind, i, none_case = case()
    check(table)                                                            # the good table passes
    shape = tuple(table[i].shape)
    assert len(shape) >= 2
    bads = {"dtype": table[i].double(), "half": table[i].half(), "strided": torch.zeros(shape + (2,))[..., 0],
            "shape": table[i].reshape(-1), "not a tensor": table[i].numpy()}
    for name, bad in bads.items():
        t2 = list(table)
        t2[i] = bad
        want = f"lbl: {kind} entry {i} is missing" if name == "not a tensor" else \
            f"lbl: {kind} entry {i} must be a contiguous float32 {shape} tensor on cpu, got "
        with pytest.raises(R.RegtError, match=re.escape(want)) as err:
            check(t2)
        assert ("(not contiguous)" in str(err.value)) == (name == "strided"), name
        if name == "shape":
            assert f"got torch.float32 {(table[i].numel(),)} on cpu" in str(err.value)
    t2 = list(table)
    t2[i] = None
    with pytest.raises(R.RegtError, match=re.escape(f"lbl: {kind} entry {i} is missing")):
        check(t2)
    if none_case is not None:
        check_off, off_table, j, reason = none_case
        check_off(off_table)                                                # the table of a module built with the switch off passes
        assert off_table[j] is None
        t2 = list(off_table)
        t2[j] = table[j]
        with pytest.raises(R.RegtError, match=re.escape(f"lbl: {kind} entry {j} must be None ({reason})")):
            check_off(t2)                                                   # present where the dims say it must be None
