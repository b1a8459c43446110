"""Every kernel form of the regional embedding h = leaky_relu(x A0^T + (L~ x) A_region^T + b') against float64, per element.

tests/embed_probe.py reads h through the public module (update gate forced to exactly 1, attention to exactly one period) on graphs
and weights whose composed operands are known exactly on the host.  Each case runs two input families: ``exact`` (every partial sum is
an fp32 and a bf16 value: h must EQUAL the expected bits, in any summation order) and ``full`` (full mantissas: op_bars.linear_ratio
against float64 <= op_bars.BAR["linear"]; forms that store h as bf16: op_bars.bf16_store_ratio <= BAR["bf16_store"]).  Each case first
proves on the device that the probe is transparent (other reset / candidate / head parameters and another x at the other periods leave
hidden bit-identical) and runs twice with identical bits.  The layouts (embed_probe.LAYOUTS) put three and more regions into a tile,
region ids without rows between two that have rows, region boundaries on tile boundaries, regions into the tail tile and the
successive tiles of a persistent workgroup into different regions; tests/test_embed_probe_cpu.py shows on the host that they do, that
the bars leave the fp32 restatement a factor of 4, and that four planted kernel errors fail both families.

embed_fp32_kernel (csrc/embed.hip) needs M = N T >= 65 536 rows: the four large layouts, each also under embed_kernel = 0 (the general
core's big tiles with SEG_REGION on the same rows).  tgnn.linear.weight is (C, R C), so a case has at most 64 regions: ``ragged`` and
``aligned`` give the rows that the cycle of small regions does not use to one large region in the middle.
Measured ratios: profiles/embed_bars.txt (tools/embed_bars.py)."""
import pytest
import torch

import embed_probe as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd
    regtgcn_amd.load_library()
    return regtgcn_amd


def _check(form, layout, m):
    print(f"{form} | {layout} | {m['stage']} | exact {'equal' if m['exact'] else 'DIFFERS'} | full r = {m['full']:.3e} (bar {m['bar']:.3e})")
    assert m["exact"], f"{form} {layout}: {m['exact_wrong_rows'].numel()} rows differ from the exact value, first {m['exact_wrong_rows'][:8].tolist()}"
    assert m["full"] <= m["bar"], (form, layout, m["full"])


@pytest.mark.parametrize("layout", E.BIG)
def test_embed_fp32_kernel_and_the_big_tile_core_per_element(R, layout):
    k = E.measure(R, "embed_fp32_kernel", layout)
    assert k["stage"] == "embed_fp32_kernel"
    _check("embed_fp32_kernel", layout, k)
    g = E.measure(R, "general-core/SEG_REGION big tiles", layout)
    assert g["stage"].startswith("general core mode 0 big tiles")
    _check("general-core/SEG_REGION big tiles", layout, g)
    assert torch.equal(k["h_exact"], g["h_exact"])


@pytest.mark.parametrize("form,layout", [(f, lay) for f, spec in E.FORMS.items() if spec[4] is not E.BIG for lay in spec[4]])
def test_every_other_form_per_element(R, form, layout):
    _check(form, layout, E.measure(R, form, layout))
