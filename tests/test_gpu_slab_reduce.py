"""The ORDER of the baselines' slab reductions (csrc/slab_reduce.h), pinned bit for bit: after a backward the scratch still holds
the partial rows the kernels summed.  Each test reads them back, adds them on the host in float32 with one elementwise add per
row in the documented order -- never torch.sum, whose order is its own -- and requires the returned gradients to be the same
BITS (int32 views: a signed zero counts).

    SpatialGCN   rows in chunks of 32 from +0, then the chunk sums from +0 (the chunk sums are in the scratch too, and checked)
    GRU          the row chunks' slabs in order, seeded with slab 0
    STID         the workgroups' slabs from +0 in workgroup order; the per-batch node-embedding rows from +0 in batch order

STNorm reuses one slab for every layer of a call, so nothing of it can be read back."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.detach().cpu().contiguous().view(-1).view(torch.int32)


def _sum_rows(rows, seed_row0=False):
    """rows (n, width) on the host, added one row at a time in row order, from +0 or from row 0."""
    acc = rows[0].clone() if seed_row0 else torch.zeros_like(rows[0])
    for r in rows[1 if seed_row0 else 0:]:
        acc = acc + r
    return acc


def _same_bits(got, want, what):
    assert got.dtype == want.dtype == torch.float32 and got.numel() == want.numel(), what
    diff = _bits(got) != _bits(want)
    assert not bool(diff.any()), (what, int(diff.sum()), int(diff.nonzero()[0]))


@pytest.mark.parametrize("n,t,f,rows,chunks", [(1120, 2, 4, 70, 3), (16, 1, 4, 1, 1)], ids=["ragged-70-rows", "one-row"])
def test_spatial_reduction_order(n, t, f, rows, chunks):
    from regtgcn_amd import ops
    gen = torch.Generator().manual_seed(n + t)
    xp, lxp = torch.randn(n, t, f, generator=gen).to(DEV), torch.randn(n, t, f, generator=gen).to(DEV)
    w0, w1 = torch.randn(64, f, generator=gen).to(DEV) * 0.5, torch.randn(64, f, generator=gen).to(DEV) * 0.5
    b, ds = torch.randn(64, generator=gen).to(DEV) * 0.2, torch.randn(n, 64, generator=gen).to(DEV)
    dw0, dw1, db, slab = ops.spatial_embed_backward(xp, lxp, w0, w1, b, None, ds, return_scratch=True)
    assert rows == (n + 15) // 16 and chunks == (rows + 31) // 32            # one wave per 16-node tile, chunks of 32 wave rows
    width = 2 * 64 * f + 64
    assert slab.numel() == (rows + chunks) * width
    slab = slab.cpu().view(rows + chunks, width)
    part = torch.stack([_sum_rows(slab[32 * c:min(32 * c + 32, rows)]) for c in range(chunks)])
    _same_bits(slab[rows:], part, "chunk sums")
    _same_bits(torch.cat([dw0.flatten(), dw1.flatten(), db]), _sum_rows(part), "dW0 | dW1 | db")
    assert float(dw0.abs().max()) > 0 and float(db.abs().max()) > 0


@pytest.mark.parametrize("seq,rows,t,chunks", [(3, 200, 3, 3), (1, 8, 3, 1)], ids=["three-chunks", "one-chunk"])
def test_gru_reduction_order(seq, rows, t, chunks):
    from regtgcn_amd import ops
    gen = torch.Generator().manual_seed(seq * 1000 + rows)
    w = [(torch.rand(shape, generator=gen) - 0.5).to(DEV) / 8 for shape in ((768, t), (768, 256), (768,), (768,))]
    x, dout = torch.randn(seq, rows, t, generator=gen).to(DEV), torch.randn(seq, rows, 256, generator=gen).to(DEV)
    h0 = (torch.randn(1, rows, 256, generator=gen) * 0.5).to(DEV)            # with one step dW_hh is the product with h0 alone
    _out, _last, dims, ws = ops.gru_forward(x, w, h0)
    grads, _dh0, sc = ops.gru_backward(dims, x, w, dout, None, ws, return_scratch=True)
    m = seq * rows
    chunk = max(256, ((m + 63) // 64 + 15) // 16 * 16)                         # rows of a chunk: at least 256
    assert chunks == (m + chunk - 1) // chunk
    width = 768 * 256 + 768
    slab = sc[sc.numel() - chunks * width:].cpu().view(chunks, width)         # the hidden gradients' slab, written last
    _same_bits(torch.cat([grads[1].flatten(), grads[3]]), _sum_rows(slab, seed_row0=True), "dW_hh | db_hh")
    assert float(grads[1].abs().max()) > 0 and float(grads[3].abs().max()) > 0


@pytest.mark.parametrize("if_node", [True, False], ids=["node-emb", "no-node-emb"])
@pytest.mark.parametrize("b,n,slabs", [(2, 130, 6), (3, 5504, 256)], ids=["six-slabs", "258-tiles-on-256-workgroups"])
def test_stid_reduction_order(b, n, slabs, if_node):
    from regtgcn_amd import ops
    dims = ops.stid_dims(n, b, 6, 8, 3, 3, 2, if_node=if_node)
    gen = torch.Generator().manual_seed(b * 10000 + n + int(if_node))
    params = [None if s is None else ((torch.rand(s, generator=gen) - 0.5) * 0.4).to(DEV) for s in ops.stid_table_shapes(dims)]
    x, dout = torch.randn(b, 6, n, 8, generator=gen).to(DEV), torch.randn(b, 2, n, 1, generator=gen).to(DEV)
    _out, ws = ops.stid_forward(dims, x, params)
    grads, sc = ops.stid_backward(dims, x, params, None, dout, ws, return_scratch=True)
    assert slabs == min(b * ((n + 63) // 64), 256)                            # a tile is 64 nodes of one batch element
    width = sum(g.numel() for g in grads[1:])
    assert sc.numel() == slabs * width + (b * n * 32 if if_node else 0)
    sc = sc.cpu()
    _same_bits(torch.cat([g.flatten() for g in grads[1:]]), _sum_rows(sc[:slabs * width].view(slabs, width)), "weight gradients")
    assert all(float(g.abs().max()) > 0 for g in grads[1:])
    if if_node:
        _same_bits(grads[0].flatten(), _sum_rows(sc[slabs * width:].view(b, n * 32)), "node_emb gradient")
    else:
        assert grads[0] is None
