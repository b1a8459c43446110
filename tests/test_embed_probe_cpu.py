"""The embedding probe (tests/embed_probe.py) checked on the host: it is transparent on the oracle, its operands are exact, the fp32
restatement stays a factor of 4 under the bar (``full``) and equals the expected bits (``exact``) on every GPU case's inputs, and the
four planted corruptions are caught by both families.  tests/test_gpu_embed_bars.py runs the same probes on the kernels."""
import pytest
import torch

import embed_probe as E
import op_bars as B
from oracle import graph_ops as G
from oracle import model as M

GPU_LAYOUTS = sorted({(lay, f, c) for _m, _o, f, c, lays in E.FORMS.values() for lay in lays})
_PROBES = {}


def probe(layout, f=32, c=256):
    if (layout, f, c) not in _PROBES:
        _PROBES[(layout, f, c)] = E.Probe(layout, f, c)
    return _PROBES[(layout, f, c)]


@pytest.mark.parametrize("layout", ["tiny", "tiny-overlap"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_the_probe_is_transparent_on_the_oracle(layout, dtype):
    """hidden == h[:, t0] exactly, for each t0 and both families, whatever the reset, candidate and head parameters are."""
    p = E.Probe(layout, f=8, c=32)
    for family in E.FAMILIES:
        x = p.x(family).to(dtype)
        a0, ar, bp = (v.to(dtype) for v in p.composed(family))
        pre = torch.einsum("nft,cf->ntc", x, a0) + bp
        for slot in range(2 if p.overlap else 1):
            lx = p.lx(x, slot)
            w = torch.where((p.reg[:, slot] >= 0)[:, None, None], ar[p.reg[:, slot].clamp_min(0)], torch.zeros(1, dtype=dtype))
            pre = pre + torch.einsum("nft,ncf->ntc", lx, w)
        h = torch.nn.functional.leaky_relu(pre, E.SLOPE)
        rw = [None if w is None else w.to(dtype) for w in p.region_weight]
        for t0 in range(p.t):
            base = None
            for variant in (0, 1):
                prm = {k: v.to(dtype) for k, v in p.params(family, t0, variant).items()}
                xv = p.x(family, variant=variant, keep=t0).to(dtype)
                _pred, hidden = M.regional_temporal_gcn(prm, xv, p.edge_index, p.region_index, rw)
                # the oracle's own h of period t0 (models/RegionalTemporalGCN.py:136-143), op for op
                per_region = [G.cheb_conv(xv[:, :, t0], ei, ew, prm["tgnn.conv.lins.0.weight"], prm["tgnn.conv.lins.1.weight"],
                                          prm["tgnn.conv.bias"]) for ei, ew in zip(p.region_index, rw)]
                own = torch.nn.functional.leaky_relu(torch.cat(per_region, dim=1) @ prm["tgnn.linear.weight"].t() + prm["tgnn.linear.bias"])
                assert torch.equal(hidden, own), (family, t0, variant)
                if family == "exact":          # ... which in the exact family is the composed form's, in any order
                    assert torch.equal(hidden, h[:, t0]), (family, t0, variant)
                else:
                    assert torch.allclose(hidden, h[:, t0], rtol=0, atol=1e-4 if dtype == torch.float32 else 1e-12), (family, t0)
                base = hidden if base is None else base
                assert torch.equal(hidden, base), (family, t0)


@pytest.mark.parametrize("layout", ["tiny", "small-5", "overlap-5", "unsorted-5", "aligned"])
def test_the_graphs_laplacians_hold_only_0_and_minus_1(layout):
    p = probe(layout)
    if p.n > 1000:                        # (a dense N x N matrix per region: the edge weights themselves at the large shapes)
        for ei, ew in zip(p.region_index, p.region_weight):
            _s, _d, w = G.cheb_norm_edges(ei, ew, p.n)
            assert bool(((w == 0) | (w == -1)).all())
        return
    total = torch.zeros(p.n, p.n)
    for r, (ei, ew) in enumerate(zip(p.region_index, p.region_weight)):
        lt = G.dense_cheb_operator(ei, ew, p.n).float()
        assert bool(((lt == 0) | (lt == -1)).all()), r
        total += lt
        x = p.x("full")[:, :, 0]
        want = sum(torch.where((p.reg[:, s] == r)[:, None], -x[p.par[:, s].clamp_min(0)], torch.zeros_like(x)) for s in range(2))
        assert torch.equal(lt @ x, want), r
    assert int((total != 0).sum()) == int((p.par >= 0).sum())


@pytest.mark.parametrize("layout,f,c", GPU_LAYOUTS)
def test_the_operands_are_exact(layout, f, c):
    """The float64 composition of A0, A_r and b' is fp32-representable and equals fp32 compositions in two summation orders; the
    exact family's sums stay inside 2^24 steps of their grid, so every partial sum in any order is an fp32 value."""
    p = probe(layout, f, c)
    for family in E.FAMILIES:
        want = p.composed(family, torch.float64)
        for order in (0, 1):
            got = p.composed(family, torch.float32, order)
            for w, g in zip(want, got):
                assert torch.equal(g.double(), w), (family, order)
    bound, grid = p.exact_bound()
    assert bound / grid <= 2.0 ** 24, (bound, grid)
    a, groups, bp = p.operands("exact")
    for t in (a, bp) + tuple(w for _r, w in groups):
        assert torch.equal(t / grid, torch.round(t / grid))
    if any(m == 2 and (f, c) == (ff, cc) and layout in lays for m, _o, ff, cc, lays in E.FORMS.values()):
        for t in (a,) + tuple(w for _r, w in groups):            # the bf16 forms round the operands: the exact family's survive it
            assert torch.equal(B.bf16_round(t), t)
    assert sum(r.numel() for r, _w in groups) == p.n * p.t


@pytest.mark.parametrize("layout,f,c", GPU_LAYOUTS)
def test_the_restatement_is_under_a_quarter_of_the_bar_and_equals_the_exact_bits(layout, f, c):
    p = probe(layout, f, c)
    assert torch.equal(p.restatement("exact"), p.expected_exact())
    r = p.full_ratio(p.restatement("full"))
    print(f"{layout} F {f} C {c}: fp32 restatement r = {r:.3e} (cap {B.BAR['linear'] / 4:.3e})")
    assert r <= B.BAR["linear"] / 4
    ariths = {m for m, _o, ff, cc, lays in E.FORMS.values() if (ff, cc) == (f, c) and layout in lays} - {0}
    for arith in sorted(ariths):
        h = p.restatement("full", arith)
        if arith == 2:
            assert torch.equal(B.bf16_round(p.restatement("exact", 2)), p.expected_exact(bf16=True))
            assert p.full_ratio(h, rounded=True) <= B.BAR["linear"] / 4
            assert p.full_ratio(B.bf16_round(h), rounded=True, stored_bf16=True) <= B.BAR["bf16_store"] / 4
        else:
            assert torch.equal(p.restatement("exact", 1), p.expected_exact())
            assert p.full_ratio(h) <= B.BAR["linear"] / 4


@pytest.mark.parametrize("name", sorted(E.CORRUPTIONS))
@pytest.mark.parametrize("layout", ["small-5", "small-1"])
def test_planted_corruptions_are_caught(layout, name):
    p = probe(layout)
    c = E.CORRUPTIONS[name](p)
    assert not torch.equal(p.restatement("exact", 0, c), p.expected_exact())
    assert p.full_ratio(p.restatement("full", 0, c)) >= 2 * B.BAR["linear"]
    hb = B.bf16_round(p.restatement("full", 2, c))
    assert not torch.equal(B.bf16_round(p.restatement("exact", 2, c)), p.expected_exact(bf16=True))
    assert p.full_ratio(hb, rounded=True, stored_bf16=True) >= 2 * B.BAR["bf16_store"]


def test_the_layouts_hold_what_they_are_for():
    """Tiles with three or more regions, a region id without rows between two that have rows, region boundaries on tile boundaries, a
    tail tile that straddles regions, successive tiles of one workgroup in different regions (256 workgroups)."""
    def owners(p):
        o = p.reg[:, 0].clone()
        last = 0
        for i in range(p.n):
            last = int(o[i]) if o[i] >= 0 else last
            o[i] = last
        return torch.repeat_interleave(o, p.t)

    rag = owners(probe("ragged"))
    tiles = [rag[i:i + 128] for i in range(0, rag.numel(), 128)]
    assert max(len(torch.unique(t)) for t in tiles) >= 3
    assert any(int(t.max() - t.min()) + 1 > len(torch.unique(t)) for t in tiles)                # an id in between owns no row
    assert any(int(tiles[b][0]) != int(tiles[b + 256][0]) for b in range(len(tiles) - 256))
    assert rag.numel() == 65544 and E.region_sorted(probe("ragged"))
    al = owners(probe("aligned"))
    change = torch.nonzero(al[1:] != al[:-1]).flatten() + 1
    assert change.numel() == 63 and bool((change % 128 == 0).all()) and al.numel() % 128 == 24
    de = owners(probe("dense"))
    assert len(torch.unique(de[:128])) >= 50 and len(torch.unique(de[199 * 128:200 * 128])) >= 2 and len(torch.unique(de[200 * 128:201 * 128])) >= 2
    assert de.numel() % 128 == 64 and len(torch.unique(de[-64:])) >= 3
    assert owners(probe("one-region")).numel() % 128 == 8
    assert not E.region_sorted(probe("unsorted-12")) and probe("overlap-5").overlap == 4


def test_every_form_is_reached_by_its_cases():
    """The dispatch of csrc/api_step.hip, restated: each form's cases select the kernel the form is named after."""
    want = {"embed_fp32_kernel": "embed_fp32_kernel", "general-core/SEG_REGION big tiles": "general core mode 0 big tiles/",
            "general-core/few tiles": "general core mode 0 few tiles/SEG_REGION", "general-core/F=7 C=128": "general core mode 0 generic/SEG_REGION",
            "general-core/bf16x3": "general core mode 1 big tiles/SEG_REGION", "general-core/SEG_REPEAT": "general core mode 0 few tiles/SEG_REPEAT",
            "bf16 three-launch": "general core bf16 fragments/SEG_REGION", "fused 64-row": "fused_forward/64 rows",
            "fused_rows=1": "fused_forward_rows/8 waves", "fused_rows=2": "fused_forward_rows/4 waves"}
    for form, (mode, options, f, c, lays) in E.FORMS.items():
        key = [k for k in want if form.startswith(k)][0]
        for lay in lays:
            p = probe(lay, f, c)
            got = E.expected_stage(mode, options, f, c, p.n, p.t, p.R, bool(p.overlap), E.region_sorted(p))
            assert got.startswith(want[key]), (form, lay, got)


def test_the_ragged_gradient_case_is_well_conditioned_and_holds_single_node_chunks():
    """tests/test_gpu_grad_scale.py "ragged-700-8-6-1": graph.region_chunks holds chunks of a single node, and the fp32 oracle's own
    ratio to float64 is at most REL / 4 on every block, so REL holds there unchanged."""
    import numpy as np

    import test_gpu_grad_scale as T
    from grad_bars import REL, block_ratios
    from regtgcn_amd.graph import node_regions, region_chunks
    case = T.CASES["ragged-700-8-6-1"][0]()
    x, _ei, ri, _rw = case.args
    own = node_regions(ri, x.shape[0])
    tab, _reg = region_chunks(own, x.shape[2])
    assert int((tab[:, 1] - tab[:, 0] == x.shape[2]).sum()) >= 2                    # chunks of one node (T rows)
    assert bool(np.all(own[1:] >= own[:-1])) and len(np.unique(own)) < case.num_regions          # sorted; some ids own no row
    rows = np.repeat(own, x.shape[2])
    assert max(len(np.unique(rows[i:i + 64])) for i in range(0, rows.size, 64)) >= 3
    want64, got32 = case.oracle_grads(torch.float64), case.oracle_grads(torch.float32)
    for _name, label, cls, err, scale in block_ratios(got32, want64, case.num_regions):
        assert err <= REL[cls] / 4 * scale, (label, err, scale)
