"""A transparent probe that reads the regional embedding h = leaky_relu(x A0^T + (L~ x) A_region^T + b') through the public module.

Test helper only (like op_bars.py).  The embedding kernels (csrc/embed.hip, the SEG_REGION / SEG_REPEAT segments of the general GEMM
core, the embedding stage of csrc/fused.hip and csrc/fused_rows.hip) have no entry point of their own; ``hidden`` of
RegionalTemporalGCN is h only after the gates, the GRU blend and the attention sum.  The probe chooses the parameters so that those
stages pass h on bit for bit:

* update gate: conv_z.lin.weight = 0, conv_z.bias = 0, linear_z.weight = 0, linear_z.bias = 40 -- the composed bias is exactly 40 and
  Z = 1 / (1 + exp(-40)) = 1.0f, so the blend fma(Z, h, (1 - Z) H~) is h (H~ is a tanh: finite);
* attention: _attention[t0] = 0, every other entry -1e4 -- the softmax gives exactly 1 and exactly 0, hidden[n] = h[n T + t0];
  T forwards, one per t0, read all of h;
* the reset and candidate parameters and the head are arbitrary (``variant`` draws others: hidden must not move).

The operands of the embedding are known exactly on the host, so the float64 reference inherits no rounding from the library's own
graph preprocessing and weight composition:

* every regional graph is a matching inside its region (pairs i <-> j, both directions, weights None or a power of 4): out-degree 1
  gives L~ entries of exactly -1, (L~ x)[i] = -x[partner]; some nodes stay unmatched (L~ x = 0).  A block of one node has no pair:
  its region id gets a self loop only (ChebConv drops it) and so owns no node -- a region id without rows between two that have rows;
* tgnn.linear.weight has the blocks Wl_r = s_r P_r, P_r a signed permutation and s_r = SCALES[r % 4] a power of two (distinct for
  neighbouring regions): A_r = Wl_r W1 = s_r P_r W1 is exact for a full-mantissa lins.1.weight;
* lins.0.weight, conv.bias and linear.bias sit on dyadic grids coarse enough that A0 = (sum_r Wl_r) W0 and b' = (sum_r Wl_r) b_c + b_l
  are exact in fp32 in any summation order (tests/test_embed_probe_cpu.py checks it on every case).

Two input families: ``exact`` (x on multiples of 2^-5 in [0, 1), lins.1.weight on multiples of 2^-6: every product and partial sum of
the contraction is fp32-exact and bf16-exact, h is one value in any order -- the assertion is EQUALITY) and ``full`` (full-mantissa
x and lins.1.weight, held to op_bars.BAR per element against float64).

The region layouts (``LAYOUTS``) are lists of node blocks; block k gets region id ``ids[k]`` (ascending unless stated).  The library
derives node_region from the regional edges (graph.node_regions): an unmatched node at the head of a block joins the block before it,
so the kernels' region boundaries need not be the blocks' -- the expected value does not care (L~ x = 0 there).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

import op_bars as B
from oracle import model as M

RAGGED_SIZES = (1, 2, 3, 5, 8, 11, 40, 300)
SCALES = (1.0, 0.5, 2.0, 0.25)
SLOPE = 0.01
FAMILIES = ("exact", "full")
MAX_REGIONS = 64                     # tgnn.linear.weight is (C, R C)
EM_ROWS = 128                        # csrc/embed.hip: rows of a tile; embed_fp32_ok needs M >= 512 tiles
EMBED_MIN_ROWS = 512 * EM_ROWS


def ragged_blocks(n: int, count: Optional[int] = None) -> List[int]:
    """Block sizes cycling through RAGGED_SIZES until n nodes are used up (the last block takes what is left); with ``count`` blocks
    the one in the middle takes the remainder instead, so that the number of regions stays at the cap."""
    if count is None:
        out, left, k = [], n, 0
        while left > 0:
            s = min(RAGGED_SIZES[k % len(RAGGED_SIZES)], left)
            out.append(s)
            left -= s
            k += 1
        return out
    half = count // 2
    head = [RAGGED_SIZES[k % 8] for k in range(half)]
    tail = [RAGGED_SIZES[k % 8] for k in range(count - half - 1)]
    big = n - sum(head) - sum(tail)
    assert big > 0
    return head + [big] + tail


def _aligned_blocks() -> List[int]:
    # 8195 nodes, T = 8: 16 nodes are one 128-row tile; every region boundary is a tile boundary, the last 3 nodes are the tail tile
    return [16] * 31 + [8192 - 62 * 16] + [16] * 31 + [3]


def _dense_blocks(n: int = 65600) -> List[int]:
    # T = 1: a tile is 128 nodes.  54 two-node regions in tile 0, 4 straddling the boundary of tiles 199 | 200, 3 in the 64-row tail tile
    a = 128 * 200 - 4 - 108
    b = 20000
    c = n - 6 - (108 + a + 8 + b)
    return [2] * 54 + [a] + [2] * 4 + [b, c] + [2] * 3


# name -> (N, T, block sizes, region ids not ascending, overlapping pairs)
LAYOUTS: Dict[str, Tuple[int, int, List[int], bool, int]] = {
    # the four shapes of embed_fp32_kernel (M = N T >= 65 536 rows); at most MAX_REGIONS regions each
    "one-region": (5462, 12, [5462], False, 0),                    # 65 544 rows, 513 tiles, a tail tile of 8 rows
    "ragged": (5462, 12, ragged_blocks(5462, MAX_REGIONS), False, 0),
    "aligned": (8195, 8, _aligned_blocks(), False, 0),
    "dense": (65600, 1, _dense_blocks(), False, 0),
    # every other form: ragged regions at 670 nodes (670 * 12 = 8040 rows: 63 row tiles, 126 tiles of the general core < 128)
    "small-1": (670, 1, ragged_blocks(670), False, 0),
    "small-5": (670, 5, ragged_blocks(670), False, 0),
    "small-12": (670, 12, ragged_blocks(670), False, 0),
    "unsorted-1": (670, 1, ragged_blocks(670), True, 0),
    "unsorted-5": (670, 5, ragged_blocks(670), True, 0),
    "unsorted-12": (670, 12, ragged_blocks(670), True, 0),
    "overlap-5": (670, 5, ragged_blocks(670), False, 4),
    "tiny": (41, 3, [1, 2, 3, 5, 8, 11, 11], False, 0),            # the oracle's transparency, host only
    "tiny-overlap": (41, 3, [1, 2, 3, 5, 8, 11, 11], False, 2),
}
BIG = ("one-region", "ragged", "aligned", "dense")


class Probe:
    """One layout at one width: the graph, the parameters and snapshots of both families, the exact operands and expected values."""

    def __init__(self, layout: str, f: int = 32, c: int = 256, seed: int = 0):
        n, t, blocks, unsorted, overlap = LAYOUTS[layout]
        assert sum(blocks) == n and len(blocks) <= MAX_REGIONS, (layout, sum(blocks), len(blocks))
        self.layout, self.n, self.t, self.f, self.c, self.blocks, self.seed = layout, n, t, f, c, blocks, seed
        self.R = len(blocks)
        g = torch.Generator().manual_seed(1000 + seed)
        ids = torch.randperm(self.R, generator=g).tolist() if unsorted else list(range(self.R))
        self.ids = ids
        # terms of node i: up to two (region, partner) pairs, -1 = none
        self.reg = torch.full((n, 2), -1, dtype=torch.long)
        self.par = torch.full((n, 2), -1, dtype=torch.long)
        self.block_region = torch.repeat_interleave(torch.tensor(ids), torch.tensor(blocks))       # nominal region of a node
        src: List[List[torch.Tensor]] = [[] for _ in range(self.R)]
        free: Dict[int, int] = {}                            # block -> one unmatched node of it
        start = 0
        for k, size in enumerate(blocks):
            r = ids[k]
            nodes = start + torch.randperm(size, generator=g)
            spare = size % 2 + (2 if size >= 40 else 0)
            m = nodes[:size - spare]
            a, b = m[0::2], m[1::2]
            if size == 1:
                src[r].append(torch.stack([nodes, nodes]))   # a self loop: the region id exists and owns no node
            else:
                src[r].append(torch.cat([torch.stack([a, b]), torch.stack([b, a])], dim=1))
                self.reg[a, 0] = self.reg[b, 0] = r
                self.par[a, 0], self.par[b, 0] = b, a
            if spare:
                free[k] = int(nodes[-1])
            start += size
        # overlapping decomposition: a matched node u of block k is matched again, in the NEXT region's graph, with a spare node v
        self.overlap = 0
        for k in sorted(free):
            if self.overlap == overlap:
                break
            if k == 0 or blocks[k - 1] < 2:
                continue
            u = int(self.par[sum(blocks[:k - 1]):sum(blocks[:k]), 0].max())          # a matched node of block k - 1
            v, r = free[k], ids[k]
            src[r].append(torch.tensor([[u, v], [v, u]]))
            self.reg[u, 1], self.par[u, 1] = r, v
            self.reg[v, 0], self.par[v, 0] = r, u
            self.overlap += 1
        assert self.overlap == overlap, (layout, self.overlap)
        self.region_index = [torch.cat(s, dim=1).contiguous() for s in src]
        # weights: None, or one power of 4 for the whole region ((w^-1/2 w) w^-1/2 is exactly 1)
        self.region_weight = [None if r % 3 == 0 else torch.full((self.region_index[r].shape[1],), (4.0, 0.25)[r % 2]) for r in range(self.R)]
        self.edge_index = torch.cat(self.region_index, dim=1).contiguous()
        # signed permutations
        self.perm = torch.stack([torch.randperm(c, generator=g) for _ in range(self.R)])
        self.sign = torch.randint(0, 2, (self.R, c), generator=g).float() * 2 - 1
        self.scale = torch.tensor([SCALES[r % 4] for r in range(self.R)])
        self._memo: Dict = {}

    # ---- parameters and snapshots -------------------------------------------------------------------------------------------------
    def _gen(self, *key) -> torch.Generator:
        return torch.Generator().manual_seed(hash((self.seed,) + key) % (1 << 31))

    def embed_params(self, family: str) -> Dict[str, torch.Tensor]:
        c, f, R = self.c, self.f, self.R
        g = self._gen(1, FAMILIES.index(family))
        wl = torch.zeros(c, R * c)
        rows = torch.arange(c)
        for r in range(R):
            wl[rows, r * c + self.perm[r]] = self.scale[r] * self.sign[r]
        # multiples of 2^-4 in [-1/8, 1/8]: A0, a sum over up to 64 regions, stays of the size of the A_r (a few large terms in a sum
        # would carry its rounding alone) and keeps 8 significant bits at the region counts of the bf16 cases
        w0 = torch.randint(-2, 3, (c, f), generator=g).float() / 16
        if family == "exact":
            w1 = torch.randint(-63, 64, (c, f), generator=g).float() / 64     # multiples of 2^-6 in (-1, 1)
        else:
            # full mantissas, magnitudes within a factor of 2 and random signs: no element's sum is carried by a few of its terms, so
            # the fp32 restatement stays a factor of 4 under the bar on every case (tests/test_embed_probe_cpu.py)
            w1 = (0.5 + 0.5 * torch.rand(c, f, generator=g)) * (torch.randint(0, 2, (c, f), generator=g).float() * 2 - 1)
        bc = torch.randint(-4, 5, (c,), generator=g).float() / 16
        bl = torch.randint(-8, 9, (c,), generator=g).float() / 16
        return {"tgnn.linear.weight": wl, "tgnn.linear.bias": bl, "tgnn.conv.lins.0.weight": w0, "tgnn.conv.lins.1.weight": w1,
                "tgnn.conv.bias": bc}

    def params(self, family: str, t0: int, variant: int = 0, out_dim: int = 1) -> Dict[str, torch.Tensor]:
        """The whole state_dict; ``variant`` redraws the reset, candidate and head parameters."""
        p = M.init_params("RegionalTemporalGCN", self.f, self.t, out_dim, num_nodes=self.n, num_regions=self.R, seed=7 + variant,
                          hidden=self.c)
        p.update(self.embed_params(family))
        q = "tgnn._base_tgcn."
        p[q + "conv_z.lin.weight"] = torch.zeros_like(p[q + "conv_z.lin.weight"])
        p[q + "conv_z.bias"] = torch.zeros_like(p[q + "conv_z.bias"])
        p[q + "linear_z.weight"] = torch.zeros_like(p[q + "linear_z.weight"])
        p[q + "linear_z.bias"] = torch.full_like(p[q + "linear_z.bias"], 40.0)
        p["tgnn._attention"] = self.attention(t0)
        return p

    def attention(self, t0: int) -> torch.Tensor:
        a = torch.full((self.t,), -1e4)
        a[t0] = 0.0
        return a

    def x(self, family: str, bf16: bool = False, variant: int = 0, keep: Optional[int] = None) -> torch.Tensor:
        """(N, F, T).  ``variant`` > 0 with ``keep`` = t0: other values at every period but t0."""
        def draw(v):
            g = self._gen(2, FAMILIES.index(family), v)
            if family == "exact":
                return torch.randint(0, 32, (self.n, self.f, self.t), generator=g).float() / 32
            # +-[0.5, 1), full mantissa: with mixed signs the partial sums stay well under sum|terms| (an equal-sign sum of 64 terms
            # carries the rounding of every addition at its full size: the k-order restatement then sits AT bar / 4)
            x = (0.5 + 0.5 * torch.rand(self.n, self.f, self.t, generator=g)) * (torch.randint(0, 2, (self.n, self.f, self.t), generator=g).float() * 2 - 1)
            return B.bf16_round(x) if bf16 else x
        x = draw(0)
        if variant:
            y = draw(variant) * 3 - 1
            y[:, :, keep] = x[:, :, keep]
            x = y
        return x

    # ---- the operands, exactly ----------------------------------------------------------------------------------------------------
    def composed(self, family: str, dtype=torch.float64, order: int = 0):
        """(A0 (C, F), A (R, C, F), b' (C)) from the fp32 parameters, composed in ``dtype``; ``order`` 1 sums the regions backwards and
        contracts from the last k."""
        p = self.embed_params(family)
        c, R = self.c, self.R
        wl = p["tgnn.linear.weight"].to(dtype)
        w0, w1 = p["tgnn.conv.lins.0.weight"].to(dtype), p["tgnn.conv.lins.1.weight"].to(dtype)
        bc, bl = p["tgnn.conv.bias"].to(dtype), p["tgnn.linear.bias"].to(dtype)
        blocks = [wl[:, r * c:(r + 1) * c] for r in range(R)]
        s = torch.zeros(c, c, dtype=dtype)
        for blk in (reversed(blocks) if order else blocks):
            s = s + blk

        def contract(u, v):                              # u (C, C) @ v (C, X), one k after the other
            acc = torch.zeros(u.shape[0], v.shape[1], dtype=dtype)
            ks = range(u.shape[1] - 1, -1, -1) if order else range(u.shape[1])
            for k in ks:
                acc = acc + u[:, k:k + 1] * v[k:k + 1]
            return acc
        a0 = contract(s, w0)
        bp = (contract(s, bc[:, None])[:, 0] + bl) if not order else (bl + contract(s, bc[:, None])[:, 0])
        # A_r = s_r P_r W1: one nonzero per row of Wl_r, exact in any arithmetic
        a = torch.stack([(self.scale[r] * self.sign[r]).to(dtype)[:, None] * w1[self.perm[r]] for r in range(R)])
        return a0, a, bp

    def lx(self, x: torch.Tensor, slot: int = 0) -> torch.Tensor:
        """(L~_r x) of the node's ``slot``-th term as (N, F, T): -x[partner], 0 without a partner."""
        par = self.par[:, slot]
        return torch.where((par >= 0)[:, None, None], -x[par.clamp_min(0)], torch.zeros_like(x))

    def operands(self, family: str, bf16: bool = False):
        """(a (M, K) fp32, groups [(row ids, w (C, K) fp32)], b' (C) fp32): row m = n T + t of h is act(a[m] . w^T + b') with the w of
        its node's group; K = 2 F, or 3 F with overlapping regions ([x | L~_r0 x | L~_r1 x] against [A0 | A_r0 | A_r1])."""
        key = ("operands", family, bf16)
        if key not in self._memo:
            x = self.x(family, bf16)
            slots = 2 if self.overlap else 1
            a = torch.cat([x] + [self.lx(x, s) for s in range(slots)], dim=1).permute(0, 2, 1).reshape(self.n * self.t, -1).contiguous()
            a0, ar, bp = (v.float() for v in self.composed(family))
            zero = torch.zeros_like(a0)
            code = (self.reg[:, 0] + 1) * (self.R + 1) + (self.reg[:, 1] + 1 if self.overlap else 0)
            groups = []
            for cd in torch.unique(code).tolist():
                nodes = torch.nonzero(code == cd).flatten()
                rows = (nodes[:, None] * self.t + torch.arange(self.t)).flatten()
                r0, r1 = cd // (self.R + 1) - 1, cd % (self.R + 1) - 1
                w = [a0, ar[r0] if r0 >= 0 else zero]
                if self.overlap:
                    w.append(ar[r1] if r1 >= 0 else zero)
                groups.append((rows, torch.cat(w, dim=1).contiguous()))
            self._memo[key] = (a, groups, bp)
        return self._memo[key]

    def expected_exact(self, bf16: bool = False) -> torch.Tensor:
        """h (M, C) of the ``exact`` family: leaky_relu of the exact sum, one fp32 multiply by 0.01f for negatives (rounded to bf16
        for the forms that store h so)."""
        key = ("expected", bf16)
        if key not in self._memo:
            a, groups, bp = self.operands("exact")
            z = torch.empty(self.n * self.t, self.c, dtype=torch.float64)
            for rows, w in groups:
                z[rows] = a[rows].double() @ w.double().t() + bp.double()
            z32 = z.float()
            assert torch.equal(z32.double(), z), "the exact family's sums must be fp32 values"
            h = B.act32(z32, 1, SLOPE)
            self._memo[key] = B.bf16_round(h) if bf16 else h
        return self._memo[key]

    def restatement(self, family: str, arith: int = 0, corrupt=(None, None)) -> torch.Tensor:
        """h (M, C) by op_bars.linear_restatement (0 fp32 in k order, 1 bf16x3, 2 bf16 operands).  ``corrupt``: a planted error,
        (edit of (a, groups) | None, edit of h | None)."""
        a, groups, bp = self.operands(family, arith == 2)
        if corrupt[0] is not None:
            a, groups = corrupt[0](a.clone(), list(groups))
        h = torch.zeros(self.n * self.t, self.c)
        for rows, w in groups:
            h[rows] = B.act32(B.linear_restatement(a[rows], w, bp, arith), 1, SLOPE)
        return h if corrupt[1] is None else corrupt[1](h)

    def full_ratio(self, h: torch.Tensor, rounded: bool = False, stored_bf16: bool = False, family: str = "full") -> float:
        """The worst per-element ratio of h (M, C) against float64, per region's rows: op_bars.linear_ratio, or for bf16-stored h
        op_bars.bf16_store_ratio over the same denominator (the |terms| carried through the activation's slope)."""
        a, groups, bp = self.operands(family, rounded)
        worst = 0.0
        for rows, w in groups:
            if not stored_bf16:
                worst = max(worst, B.linear_ratio(h[rows], a[rows], w, bp, act=1, slope=SLOPE, rounded=rounded))
                continue
            z, den = B.linear_reference(a[rows], w, bp, rounded)
            low = float(torch.tensor(SLOPE, dtype=torch.float32))
            local = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, low))
            local = torch.where(z.abs() <= B.BAR["linear"] * den, torch.ones_like(z), local)
            worst = max(worst, B.bf16_store_ratio(h[rows], (B.act64(z, 1, SLOPE), local * den)))
        return worst

    def exact_bound(self) -> Tuple[float, float]:
        """(largest sum_k |term| + |bias| of the exact family, its grid): every partial sum in any order is a multiple of the grid below
        that magnitude, so it is an fp32 value when bound / grid <= 2^24."""
        a, groups, bp = self.operands("exact")
        worst = 0.0
        for rows, w in groups:
            worst = max(worst, float((a[rows].double().abs() @ w.double().abs().t() + bp.double().abs()).max()))
        # x: 2^-5; A_r: min scale 2^-2 x 2^-6; A0: 2^-2 x 2^-4; b': 2^-2 x 2^-4
        return worst, 2.0 ** -13

    def boundary_node(self) -> int:
        """A matched node whose successor is matched in another region (a region boundary both sides of which carry an L~ x)."""
        r = self.reg[:, 0]
        ok = (r[:-1] >= 0) & (r[1:] >= 0) & (r[:-1] != r[1:])
        return int(torch.nonzero(ok).flatten()[0])


# ---- planted corruptions of the restatement (tests/test_embed_probe_cpu.py): (edit of the operands | None, edit of h | None) ---------

def _retarget(groups, row: int, to_group_of: int):
    """Move ``row`` into the group (the weights) of row ``to_group_of``."""
    out, moved = [], False
    for rows, w in groups:
        keep = rows[rows != row]
        if bool((rows == to_group_of).any()) and not bool((rows == row).any()):
            keep = torch.cat([keep, torch.tensor([row])])
            moved = True
        out.append((keep, w))
    assert moved
    return out


def corrupt_neighbour_weights(p: Probe):
    """One row takes the neighbouring region's A_r: period 0 of the node in front of a region boundary, weights of the node behind it."""
    i = p.boundary_node()
    return (lambda a, groups: (a, _retarget(groups, i * p.t, (i + 1) * p.t))), None


def corrupt_lost_kstep(p: Probe, block: int = 1, step: int = 9):
    """One 16-row block loses one k step: 4 of the 64 products (rows 16 block .. + 15, k = 4 step .. + 3)."""
    def f(a, groups):
        a[16 * block:16 * block + 16, 4 * step:4 * step + 4] = 0.0
        return a, groups
    return f, None


def corrupt_swapped_rows(p: Probe, r0: int = 3, r1: int = 77):
    """Two rows of one 128-row tile are stored in each other's place."""
    def f(h):
        h[[r0, r1]] = h[[r1, r0]]
        return h
    return None, f


def corrupt_boundary_off_by_one(p: Probe):
    """A pass's last row ``hi`` is one too small: the last row of the region in front of a boundary is never stored (it stays 0)."""
    row = p.boundary_node() * p.t + p.t - 1

    def f(h):
        h[row] = 0.0
        return h
    return None, f


CORRUPTIONS = {"neighbour-weights": corrupt_neighbour_weights, "lost-k-step": corrupt_lost_kstep, "swapped-rows": corrupt_swapped_rows,
               "boundary-off-by-one": corrupt_boundary_off_by_one}


# ---- the forms and the dispatch that reaches them, restated (csrc/api_step.hip forward_impl / forward_bf16_rows, embed.hip) ------------

# form -> (GEMM mode, ((option, value), ...), F, C, layouts)
FORMS = {
    "embed_fp32_kernel": (0, (), 32, 256, BIG),
    "general-core/SEG_REGION big tiles": (0, ((b"embed_kernel", 0),), 32, 256, BIG),
    "general-core/few tiles": (0, (), 32, 256, ("small-1", "small-5", "small-12")),
    "general-core/F=7 C=128": (0, (), 7, 128, ("small-1", "small-5", "small-12")),
    "general-core/bf16x3": (1, (), 32, 256, ("small-1", "small-5", "small-12")),
    "general-core/SEG_REPEAT": (0, (), 32, 256, ("overlap-5",)),
    "bf16 three-launch F=32": (2, ((b"xbf", 0),), 32, 256, ("small-1", "small-5", "small-12")),
    "bf16 three-launch F=64": (2, ((b"xbf", 0),), 64, 256, ("small-1", "small-5", "small-12")),
    "fused 64-row F=32": (2, (), 32, 256, ("unsorted-12",)),
    "fused 64-row F=64": (2, (), 64, 256, ("unsorted-1", "unsorted-5", "unsorted-12")),
    "fused_rows=1 F=32": (2, ((b"fused_rows", 1),), 32, 256, ("small-12",)),
    "fused_rows=1 F=64": (2, ((b"fused_rows", 1),), 64, 256, ("small-1", "small-5", "small-12")),
    "fused_rows=2 F=32": (2, ((b"fused_rows", 2),), 32, 256, ("small-12",)),
    "fused_rows=2 F=64": (2, ((b"fused_rows", 2),), 64, 256, ("small-1", "small-5", "small-12")),
}


def region_sorted(p: Probe) -> bool:
    """graph.node_regions + PreparedGraph.region_sorted, restated: unowned nodes join the last owned node before them."""
    owner = p.reg[:, 0].clone()
    last = 0
    for i in range(p.n):
        if owner[i] < 0:
            owner[i] = last
        last = int(owner[i])
    return bool((owner[1:] >= owner[:-1]).all())


def expected_stage(mode: int, options: Sequence, f: int, c: int, n: int, t: int, R: int, overlap: bool, sorted_: bool) -> str:
    """Which kernel computes h, from the host-side predicates of csrc/api_step.hip (default environment)."""
    o = {b"embed_kernel": 1, b"xbf": 1, b"fused_rows": 1}
    o.update(dict(options))
    m = n * t
    ibf = mode == 2 and c % 128 == 0 and f % 4 == 0                                   # bf16_intermediates
    frag = ibf and f % 32 == 0                                                        # frag_shape_ok
    if frag and o[b"xbf"] and R > 1 and not overlap and c == 256 and f in (32, 64) and (t * f) % 64 == 0:      # xbf_ok, fused_forward_ok
        if o[b"fused_rows"] and t <= 16 and (R == 1 or sorted_):                      # fused_rows_form
            return f"fused_forward_rows/{4 if o[b'fused_rows'] == 2 else 8} waves"
        return "fused_forward/64 rows"
    if mode == 0 and o[b"embed_kernel"] and not overlap and (R == 1 or sorted_) and c == 256 and f == 32 and m >= EMBED_MIN_ROWS:
        return "embed_fp32_kernel"
    seg = "SEG_REPEAT" if overlap else ("SEG_REGION" if R > 1 else "one region")
    if frag and not overlap and (min(R, 128 // t + 2) + 1) * (f // 32) <= 64 and (2 * c + f) // 32 <= 64:   # weights_frag
        return f"general core bf16 fragments/{seg}"
    tiles = -(-m // 128) * -(-c // 128)
    vec = f % 4 == 0
    size = "generic" if not vec else ("few tiles" if mode == 0 and tiles < 128 else "big tiles")
    return f"general core mode {mode} {size}/{seg}"


# ---- the probe on the device (tests/test_gpu_embed_bars.py, tools/embed_bars.py) ----------------------------------------------------

_PROBES: Dict = {}


def probe(layout: str, f: int = 32, c: int = 256) -> Probe:
    if (layout, f, c) not in _PROBES:
        _PROBES[(layout, f, c)] = Probe(layout, f, c)
    return _PROBES[(layout, f, c)]


def read_h(R, p: Probe, family: str, bf16: bool, periods=None, variant: int = 0) -> torch.Tensor:
    """h (M, C) on the host, read through RegionalTemporalGCN: one forward per period t0 (``periods``: only those; the other rows stay
    NaN).  ``variant``: other reset, candidate and head parameters and another x at every period but t0."""
    dev = "cuda"
    ei = p.edge_index.to(dev)
    ri = [i.to(dev) for i in p.region_index]
    rw = [None if w is None else w.to(dev) for w in p.region_weight]
    mod = R.RegionalTemporalGCN(node_features=p.f, num_nodes=p.n, periods=p.t, output_dim=1, num_regions=p.R, hidden_channels=p.c)
    mod.load_state_dict(p.params(family, 0, variant), strict=True)
    mod = mod.to(dev)
    h = torch.full((p.n, p.t, p.c), float("nan"), device=dev)
    x = None if variant else p.x(family, bf16).to(dev)
    for t0 in (range(p.t) if periods is None else periods):
        with torch.no_grad():
            mod.tgnn._attention.copy_(p.attention(t0).to(dev))
        xv = p.x(family, bf16, variant, keep=t0).to(dev) if variant else x
        _pred, hidden = mod(xv, ei, ri, rw)                  # (parameters require grad: the training forward, not the forward-only one)
        h[:, t0] = hidden.detach()
    torch.cuda.synchronize()
    return h.reshape(p.n * p.t, p.c).cpu()


def measure(R, form: str, layout: str):
    """One form on one layout, both families: asserts transparency on the device and identical bits in a second run; returns
    {"exact": h == expected bit for bit, "h_exact": h, "full": worst ratio, "bar": its bar, "stage": the kernel the dispatch selects}."""
    mode, options, f, c, _lays = FORMS[form]
    p = probe(layout, f, c)
    lib = R.load_library()
    prev_mode = lib.regt_set_gemm_mode(mode)
    prev = [(opt, lib.regt_set_option(opt, val)) for opt, val in options]
    bf16 = mode == 2
    out = {"stage": expected_stage(mode, options, f, c, p.n, p.t, p.R, bool(p.overlap), region_sorted(p))}
    try:
        for family in FAMILIES:
            h = read_h(R, p, family, bf16)
            assert bool(torch.isfinite(h).all()), (form, layout, family)
            assert torch.equal(read_h(R, p, family, bf16), h), f"{form} {layout} {family}: two runs differ"
            ends = sorted({0, p.t - 1})
            hv = read_h(R, p, family, bf16, periods=ends, variant=1).reshape(p.n, p.t, p.c)[:, ends]
            assert torch.equal(hv, h.reshape(p.n, p.t, p.c)[:, ends]), f"{form} {layout} {family}: the probe is not transparent"
            if bf16:
                assert torch.equal(B.bf16_round(h), h), f"{form} {layout}: h is expected as bf16 values"
            if family == "exact":
                out["h_exact"] = h
                out["exact"] = torch.equal(h, p.expected_exact(bf16))
                out["exact_wrong_rows"] = torch.nonzero((h != p.expected_exact(bf16)).any(dim=1)).flatten()
            else:
                out["full"] = p.full_ratio(h, rounded=bf16, stored_bf16=bf16)
                out["bar"] = B.BAR["bf16_store" if bf16 else "linear"]
    finally:
        for opt, val in reversed(prev):
            lib.regt_set_option(opt, val)
        lib.regt_set_gemm_mode(prev_mode)
    return out
