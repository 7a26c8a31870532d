"""The kernels of csrc/augment.hip at their own boundaries ("Pinned edges of random_prop and the embedding
bag"): staging passes and the 8-wide unroll (A), sample chunks (B), VEC and feature slabs (C), the second trip of the
grid-stride loops (D), COO segments round the 1 024-entry stage and `n_out` (E), scores that vanish in float32 (F), and
the embedding bag's lane groups and read rounds (G).  Reference: oracle.random_prop_ref and emb_ref in float64, autograd
for the gradients, under explicit masks; tolerance per element |d| <= 1e-5 * sum|terms| + 1e-7 (`close`), the same for
every case.  Bitwise contracts (S-sample = single calls, CSR = COO, cut = uncut prefix) are compared with torch.equal.
The cases carry sentinels (augment_cases.py): tests/test_host_augment_edges.py shows that the tolerance sees the loss of
any one of them and that float32 in the kernels' order stays inside it."""
import pytest

import augment_cases as ac
from augment_cases import close

pytestmark = pytest.mark.gpu


def _rows_call(c, x, training, S=None, keep=None, deterministic=False):
    """random_prop_rows on the case: S = None follows the case (S = 1: the single-sample entry); keep [S, R * K]."""
    from grand_plus_amd.augment import random_prop_rows
    S = c.S if S is None else S
    keep = (c.keep.reshape(c.S, -1) if keep is None else keep).cuda()
    return random_prop_rows(x, c.col.reshape(-1).cuda(), c.val.reshape(-1).cuda(), c.filled.cuda(), c.K, batch_rows=c.rows.cuda(),
                            dropnode_rate=c.p, training=training, keep=keep if S > 1 else keep[0].contiguous(), samples=S,
                            deterministic=deterministic)


def _coo_call(v, x, training, S=None, keep=None, n_out=None):
    from grand_plus_amd.augment import random_prop
    S = v.S if S is None else S
    keep = (v.keep if keep is None else keep).cuda()
    return random_prop(x, v.scores.cuda(), v.idx.cuda(), v.p, training=training, keep=keep if S > 1 else keep[0].contiguous(),
                       samples=S, n_out=v.n_out if n_out is None else n_out)


def _shaped(out, S):
    return out if S > 1 else out[None]


def _check_rows(c, training, deterministic=(False, True), coo=False, tail=0):
    """Forward and backward(s) of the fused form against float64; with coo the same batch through the COO form
    (feats = X[cols]).  tail > 0: the last `tail` output rows are compared on their own as well."""
    import torch
    v = ac.coo_view(c)
    ref, terms = ac.coo_reference(v, training)
    gref, gterms = ac.coo_ref_grad(v, training, c.X) if v.idx.numel() else (torch.zeros(c.N, c.F),) * 2
    G = (c.G if c.S > 1 else c.G[0]).cuda()
    out = None
    for det in deterministic:
        x = c.X.cuda().requires_grad_(True)
        out = _rows_call(c, x, training, deterministic=det)
        assert out.shape == ref.shape[1 - (c.S > 1):] and out.grad_fn is not None
        close(_shaped(out, c.S), ref, terms)
        out.backward(G)
        close(x.grad, gref, gterms)
        named = torch.zeros(c.N, dtype=torch.bool); named[v.cols] = True
        assert torch.count_nonzero(x.grad.cpu()[~named]) == 0                      # nodes of no filled slot: exact zeros
    empty = (c.filled[c.rows.long()] == 0).nonzero().flatten()
    assert torch.count_nonzero(_shaped(out, c.S)[:, empty.cuda()]) == 0          # the empty rows
    if tail:
        close(_shaped(out, c.S)[:, -tail:], ref[:, -tail:], terms[:, -tail:])
    if coo and v.idx.numel():
        f = v.feats.cuda().requires_grad_(True)
        o = _coo_call(v, f, training)
        close(_shaped(o, c.S), ref, terms)
        o.backward(G)
        cref, cterms = ac.coo_ref_grad(v, training)
        close(f.grad, cref, cterms)
        if tail:
            last = v.idx >= v.n_out - tail
            close(_shaped(o, c.S)[:, -tail:], ref[:, -tail:], terms[:, -tail:])
            close(f.grad[last.cuda()], cref[last], cterms[last])
    return out


@pytest.mark.parametrize("K", ac.A_K)
@pytest.mark.parametrize("F", [12, 65])
@pytest.mark.parametrize("S", [1, 2])
def test_k_edges_rows_form(K, F, S):
    """A: one to four staging passes of 256 entries into the 1 024-entry stage, and the unrolled loop's last full trip and
    tail (n = 8q - 1, 8q, 8q + 1), with filled in {K, 1, 0, 8 * (K // 8), K - 1, K + 5} and one row named twice."""
    import torch
    for training in (False, True):
        c = ac.edge_rows(K, F, S, seed=K + F + S)
        _check_rows(c, training)
    keep = c.keep.clone()
    keep[:, 0] = 0                                                                  # resident row 0: batch rows 1 and 4
    out = _shaped(_rows_call(c, c.X.cuda(), True, keep=keep.reshape(S, -1)), S)
    assert torch.count_nonzero(out[:, [1, 4]]) == 0 and torch.count_nonzero(out[:, 6]) > 0   # all dropped: exactly 0


@pytest.mark.parametrize("K", ac.B_K)
@pytest.mark.parametrize("S", ac.B_S)
def test_sample_chunks_rows_form(K, S):
    """B: the forward takes chunks of at most 8 samples (S = 9: 8 + 1, S = 15: 8 + 7, S = 16: 8 + 8; S in {5, 7} run 8
    accumulators with ns < NS).  The backward's chunk is rows_nsc(K, S, 16) = min(S, (16 384 - K - 16) // K) samples: 14 at
    K = 1 024 and 15 at K = 963, so it takes two chunks, and a second atomic per element, at (K, S) = (1 024, 15),
    (1 024, 16) and (963, 16); every other pair here takes one."""
    import torch
    c = ac.edge_rows(K, 65, S, seed=3 * K + S)
    out = _check_rows(c, True, deterministic=(False,))
    x = c.X.cuda()
    for s in range(S):
        one = _rows_call(c, x, True, S=1, keep=c.keep[s].reshape(1, -1))
        assert torch.equal(out[s], one), f"sample {s} differs from the single call with keep[{s}]"
    from grand_plus_amd.augment import random_prop_rows, sample_seed
    args = (x, c.col.reshape(-1).cuda(), c.val.reshape(-1).cuda(), c.filled.cuda(), K)
    seeded = random_prop_rows(*args, batch_rows=c.rows.cuda(), dropnode_rate=c.p, training=True, seed=991 + S, samples=S)
    for s in range(S):
        one = random_prop_rows(*args, batch_rows=c.rows.cuda(), dropnode_rate=c.p, training=True, seed=sample_seed(991 + S, s))
        assert torch.equal(seeded[s], one), f"sample {s} differs from the single call with sample_seed"


def _check_coo(c, training):
    """Forward and backward of the COO form against float64; returns (out [S, n_out, F], gradient)."""
    ref, terms = ac.coo_reference(c, training)
    f = c.feats.cuda().requires_grad_(True)
    out = _coo_call(c, f, training)
    close(_shaped(out, c.S), ref, terms)
    out.backward((c.G if c.S > 1 else c.G[0]).cuda())
    close(f.grad, *ac.coo_ref_grad(c, training))
    return _shaped(out, c.S), f.grad


@pytest.mark.parametrize("S", ac.B_COO_S)
def test_sample_chunks_coo_form(S):
    """B: the COO forward's chunks of 8 samples over E's segments (1 023 and 1 024 staged, 1 025 on the plain loop)."""
    import torch
    from grand_plus_amd.augment import random_prop, sample_seed
    c = ac.edge_coo(6, S, seed=40 + S)
    out, _ = _check_coo(c, True)
    f, sc, ix = c.feats.cuda(), c.scores.cuda(), c.idx.cuda()
    seeded = random_prop(f, sc, ix, c.p, training=True, seed=17 + S, samples=S, n_out=c.n_out)
    for s in range(S):
        assert torch.equal(out[s], _coo_call(c, f, True, S=1, keep=c.keep[s:s + 1]))
        assert torch.equal(seeded[s], random_prop(f, sc, ix, c.p, training=True, seed=sample_seed(17 + S, s), n_out=c.n_out))


@pytest.mark.parametrize("F", ac.C_F)
@pytest.mark.parametrize("S", [1, 3])
def test_widths_both_forms(F, S):
    """C: VEC = 1, 2 and 4 below one vector's worth of columns (F in {1, 2, 3, 4, 6}), a full VEC = 4 slab (1 024), a
    second slab of one live lane (1 028), three VEC = 2 slabs (1 030) and six VEC = 1 slabs (1 433)."""
    import torch
    for training in (False, True):
        c = ac.edge_rows(9, F, S, seed=F + S)
        out = _check_rows(c, training, coo=True)
    if S > 1:
        v = ac.coo_view(c)
        o = _coo_call(v, v.feats.cuda(), True)
        for s in range(S):
            assert torch.equal(out[s], _rows_call(c, c.X.cuda(), True, S=1, keep=c.keep[s].reshape(1, -1)))
            assert torch.equal(o[s], _coo_call(v, v.feats.cuda(), True, S=1, keep=v.keep[s:s + 1]))


@pytest.mark.parametrize("S", [1, 2])
def test_second_grid_trip(S):
    """D: 65 535 + 41 output rows: rows 65 535 .. 65 575 are the second trip of the first 41 workgroups, which reuse
    their LDS stage.  All four kernels of either kind (S = 1 single-sample, S = 2 S-sample); K = 2, F = 4."""
    c = ac.second_trip_rows(S)
    _check_rows(c, True, deterministic=(False,), coo=True, tail=41)


@pytest.mark.parametrize("S", [1, 2])
def test_coo_segments_and_trailing_rows(S):
    """E: segments of 1 023, 1 024 and 1 025 entries after two empty rows; n_out = mat_idx[-1] + 4 adds three zero rows
    to every sample and changes no bit of the rest nor of the gradient."""
    import torch
    for training in (False, True):
        c = ac.edge_coo(6, S, seed=40 + S)
        assert int(c.idx[0]) == 2
        out, grad = _check_coo(c, training)
        assert torch.count_nonzero(out[:, [0, 1, 5]]) == 0
        f = c.feats.cuda().requires_grad_(True)
        more = _shaped(_coo_call(c, f, training, n_out=c.n_out + 3), S)
        assert more.shape == (S, c.n_out + 3, 6) and torch.equal(more[:, :c.n_out], out)
        assert torch.count_nonzero(more[:, c.n_out:]) == 0
        G = torch.cat([c.G, torch.randn(S, 3, 6)], 1).cuda()
        more.backward(G)
        assert torch.equal(f.grad, grad)


def test_coo_without_entries():
    """E: M = 0 with n_out = 3 and S = 2 gives zeros [2, 3, F]."""
    import torch
    from grand_plus_amd.augment import random_prop
    f = torch.zeros((0, 6), device="cuda", requires_grad=True)
    out = random_prop(f, torch.zeros(0, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), 0.5, training=True,
                      seed=1, samples=2, n_out=3)
    assert out.shape == (2, 3, 6) and torch.count_nonzero(out) == 0
    out.sum().backward()
    assert f.grad.shape == (0, 6)
    one = random_prop(f.detach(), torch.zeros(0, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), 0.5, n_out=3)
    assert one.shape == (3, 6) and torch.count_nonzero(one) == 0


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("n_out", [9, 4, 3, 2, 0])
def test_coo_n_out_below_the_last_segment(S, n_out):
    """E: a caller's n_out below mat_idx[-1] + 1 cuts the entries of rows >= n_out: the forward is the uncut call's first
    n_out rows bit for bit, the gradient of the kept entries the uncut call's under the same upstream rows, and the
    gradient of every cut entry exactly 0 (n_out = 9 cuts the last segment, 4 and 3 between the long ones, 2 and 0 every
    entry).  The gradient buffer is not zeroed by the caller: a block of NaN of its size is freed just before."""
    import torch
    c = ac.edge_coo(6, S, seed=40 + S)
    kept = (c.idx < n_out).cuda()
    f = c.feats.cuda().requires_grad_(True)
    full = _shaped(_coo_call(c, f, True), S)
    G = c.G.clone()
    G[:, n_out:] = 0
    full.backward(G.cuda())
    want = f.grad.clone()
    assert torch.count_nonzero(want[~kept]) == 0 and (n_out < 3 or torch.count_nonzero(want[kept]) > 0)
    f.grad = None
    cut = _shaped(_coo_call(c, f, True, n_out=n_out), S)
    assert cut.shape == (S, n_out, 6) and torch.equal(cut, full[:, :n_out])
    poison = torch.full((c.idx.numel(), 6), float("nan"), device="cuda")
    del poison
    cut.backward(c.G[:, :n_out].cuda())
    assert torch.equal(f.grad[kept], want[kept])
    assert torch.count_nonzero(f.grad[~kept]) == 0 and not torch.isnan(f.grad).any()


@pytest.mark.parametrize("S", [1, 2])
def test_scores_that_vanish_in_float32(S):
    """F: val of 1e-60 (0 in float32) beside normal scores; a row of nothing else is a zero row with a zero gradient and
    no NaN; a row of 1e-13 throughout has den of the size of the 1e-12 epsilon.  K = 9, F = 12."""
    import torch
    for training in (False, True):
        c = ac.score_rows(S)
        out = _shaped(_check_rows(c, training), S)
        assert not torch.isnan(out).any()
        assert torch.count_nonzero(out[:, [3, 7]]) == 0 and torch.count_nonzero(out[:, 0]) > 0
    c2 = ac.score_rows(S)
    c2.rows = torch.tensor([2, 2], dtype=torch.int32)                               # the vanishing row alone
    c2.G = c2.G[:, :2]
    x = c2.X.cuda().requires_grad_(True)
    _rows_call(c2, x, True).backward((c2.G if S > 1 else c2.G[0]).cuda())
    assert torch.count_nonzero(x.grad) == 0


def _bag_call(c, W, training, deterministic):
    from grand_plus_amd.embedding import embedding_bag
    return embedding_bag(W, c.attr_idx.cuda(), c.node_idx.cuda(), c.attr_data.cuda(), input_droprate=c.p, training=training,
                         keep=c.keep.reshape(-1).cuda(), deterministic=deterministic)


@pytest.mark.parametrize("H", ac.G_H)
@pytest.mark.parametrize("training", [False, True])
def test_embedding_bag_lane_groups_and_bag_lengths(H, training):
    """G: lane groups G = 1 .. 64 (log2g 0-6) under every VEC, n_f up to 9 at G = 64, and bags of G - 1, G and G + 1
    entries for each G, 63 | 64 | 65 and 127 | 128 | 129 for the backward's 64-entry read round, two empty bags and a
    long one; forward and W.grad of both backwards against emb_ref in float64."""
    import torch
    c = ac.edge_bags(H, seed=H)
    ref, terms, dW, dW_terms = ac.bag_reference(c, training)
    for det in (False, True):
        W = c.W.cuda().requires_grad_(True)
        out = _bag_call(c, W, training, det)
        assert out.shape == ref.shape and out.grad_fn is not None
        close(out, ref, terms)
        assert torch.count_nonzero(out[[0, 21]]) == 0                             # the empty bags
        out.backward(c.G.cuda())
        close(W.grad, dW, dW_terms)
        named = torch.zeros(c.V, dtype=torch.bool); named[c.attr_idx] = True
        assert int((~named).sum()) >= 50 and torch.count_nonzero(W.grad.cpu()[~named]) == 0


@pytest.mark.parametrize("H", ac.TINY_BAG_H)
@pytest.mark.parametrize("training", [False, True])
def test_embedding_bag_weights_at_the_epsilons_scale(H, training):
    """A bag of 9 weights of 1e-11: its denominator is of the size of the 1e-10 beside it, so 1 / (den + 1e-10) is about half
    of 1 / den and a hundredth of what random_prop's 1e-12 would give; forward and W.grad of both backwards."""
    import torch
    c = ac.tiny_bags(H)
    ref, terms, dW, dW_terms = ac.bag_reference(c, training)
    assert 0.4 < float(c.attr_data[c.node_idx == ac.TINY_BAG].double().sum()) / 1e-10 / 2 < 0.5
    for det in (False, True):
        W = c.W.cuda().requires_grad_(True)
        out = _bag_call(c, W, training, det)
        close(out, ref, terms)
        assert torch.count_nonzero(out[ac.TINY_BAG]) > 0
        out.backward(c.G.cuda())
        close(W.grad, dW, dW_terms)


@pytest.mark.parametrize("H", ac.G_CSR_H)
def test_embedding_bag_csr_equals_coo_bitwise_at_the_edges(H):
    """G: the CSR form (int32 ids, nodes out of order with one repeat) equals the COO form of the same bags bit for bit."""
    import torch
    from grand_plus_amd.embedding import embedding_bag, embedding_bag_csr
    c = ac.edge_bags(H, seed=H)
    indptr, indices, data, nodes, attr_idx, node_idx, attr_data = ac.bags_as_csr(c)
    W = c.W.cuda()
    for training, seed in ((True, 4242), (False, 1)):
        coo = embedding_bag(W, attr_idx.cuda(), node_idx.cuda(), attr_data.cuda(), input_droprate=c.p, training=training, seed=seed,
                            n_out=nodes.numel())
        csr = embedding_bag_csr(W, indptr.cuda(), indices.cuda(), data.cuda(), nodes=nodes.cuda(), input_droprate=c.p,
                                training=training, seed=seed)
        assert csr.shape == (nodes.numel(), H) and torch.equal(csr, coo) and torch.count_nonzero(csr) > 0
