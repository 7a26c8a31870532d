"""CPU companion of tests/test_gpu_augment_edges.py ("Pinned edges of random_prop and the embedding bag"):
the cases of augment_cases.py themselves.  For every case a numpy float32 restatement in the kernels' order (den left to
right, inv = 1 / (den + eps), each column's sum left to right with the product rounded before the add, then * inv; the
backward (g * inv) * w summed over s) stays inside |d| <= 1e-5 * sum|terms| + 1e-7 against the float64 reference with
the largest ratio of error to bound below 0.5, so the GPU suite cannot fail on rounding and cannot pass by luck; and
taking any single sentinel entry out of the float64 reference moves some element by more than 10 bounds, so no kernel can
lose one unseen.  The measured maxima per group are in DESIGN §7e."""
import pytest
import torch

import augment_cases as ac

ROOM, SEEN = 0.5, 10.0


def _rows_ratios(c, training, backward=True):
    """Largest error-to-bound ratio of the float32 restatement over the forward, the COO gradient and the fused gradient."""
    v = ac.coo_view(c)
    ref, terms = ac.coo_reference(v, training)
    worst = ac.ratio(ac.f32_random_prop(v, training)[0], ref, terms)
    if backward and v.idx.numel():
        worst = max(worst, ac.ratio(ac.f32_random_prop_grad(v, training), *ac.coo_ref_grad(v, training)),
                    ac.ratio(ac.f32_random_prop_grad(v, training, c.N), *ac.coo_ref_grad(v, training, c.X)))
    return worst, ac.sentinel_margin(v, training)


def _check(worst, margin):
    assert worst < ROOM, f"float32 restatement uses {worst:.3f} of the bound"
    assert margin > SEEN, f"a sentinel moves the reference by only {margin:.2f} bounds"


def test_sentinel_slots_sit_where_the_kernels_change_trips():
    assert ac.sentinel_slots(0) == []
    assert ac.sentinel_slots(1) == [0]
    assert ac.sentinel_slots(9) == [0, 7, 8]
    assert ac.sentinel_slots(257) == [0, 255, 256]
    assert ac.sentinel_slots(1023) == [0, 255, 256, 511, 512, 767, 768, 1015, 1016, 1022]
    assert ac.sentinel_slots(1024) == [0, 255, 256, 511, 512, 767, 768, 1023]
    assert ac.bag_sentinel_slots(65) == [0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64]
    c = ac.edge_rows(1024, 12, 2, seed=1)
    assert c.filled.tolist() == [1024, 1, 0, 1024, 1023, 1029] and c.rows.tolist().count(0) == 2
    others = c.val[~c.sent & (torch.arange(1024)[None] < c.filled[:, None])]
    assert float(others.max()) <= 0.25 and bool((c.val[c.sent] == 1.0).all())
    assert float(c.X[:ac.N_SENT].abs().min()) >= 1.0
    assert bool((c.keep.sum(0)[c.sent] >= 1).all())                                 # every sentinel kept in some sample
    for r in range(6):                                                              # on nodes of its own within the row
        n = min(int(c.filled[r]), 1024)
        ids = c.col[r, :n][c.sent[r, :n]].tolist()
        assert len(set(ids)) == len(ids) and not set(ids) & set(c.col[r, :n][~c.sent[r, :n]].tolist())


@pytest.mark.parametrize("K", ac.A_K)
@pytest.mark.parametrize("F", [12, 65])
@pytest.mark.parametrize("S", [1, 2])
def test_group_a_k_edges(K, F, S):
    for training in (False, True):
        _check(*_rows_ratios(ac.edge_rows(K, F, S, seed=K + F + S), training))


@pytest.mark.parametrize("K", ac.B_K)
@pytest.mark.parametrize("S", ac.B_S)
def test_group_b_sample_chunks_rows(K, S):
    _check(*_rows_ratios(ac.edge_rows(K, 65, S, seed=3 * K + S), True))


@pytest.mark.parametrize("S", ac.B_COO_S + (1, 2))
def test_groups_b_and_e_coo_segments(S):
    for training in (False, True):
        c = ac.edge_coo(6, S, seed=40 + S)
        ref, terms = ac.coo_reference(c, training)
        worst = max(ac.ratio(ac.f32_random_prop(c, training)[0], ref, terms),
                    ac.ratio(ac.f32_random_prop_grad(c, training), *ac.coo_ref_grad(c, training)))
        _check(worst, ac.sentinel_margin(c, training))


@pytest.mark.parametrize("F", ac.C_F)
@pytest.mark.parametrize("S", [1, 3])
def test_group_c_widths(F, S):
    for training in (False, True):
        _check(*_rows_ratios(ac.edge_rows(9, F, S, seed=F + S), training))


@pytest.mark.parametrize("S", [1, 2])
def test_group_d_second_grid_trip(S):
    c = ac.second_trip_rows(S)
    assert c.rows.numel() == 65535 + 41 and set(c.filled.tolist()) == {0, 1, 2}
    _check(*_rows_ratios(c, True))


@pytest.mark.parametrize("S", [1, 2])
def test_group_f_scores(S):
    c = ac.score_rows(S)
    v = ac.coo_view(c)
    assert float(v.scores[v.idx == 3].max()) == 0.0                                 # 1e-60 is 0 in float32 (batch row 3 = row 2)
    assert 0.0 < float(v.scores[v.idx == 0].sum()) < 2e-12                          # batch row 0 = row 3: den of the epsilon's size
    for training in (False, True):
        _check(*_rows_ratios(c, training))
        assert not ac.f32_random_prop(v, training)[0].any(axis=(0, 2))[[3, 7]].any()   # the zero rows, no NaN
        assert not torch.isnan(torch.from_numpy(ac.f32_random_prop_grad(v, training, c.N))).any()


@pytest.mark.parametrize("H", ac.G_H)
def test_group_g_bags(H):
    c = ac.edge_bags(H, seed=H)
    assert c.attr_idx.numel() == sum(ac.G_LENS) and float(c.attr_data[~c.sent].max()) <= 0.25
    assert int((c.attr_data == 0).sum()) > 50 and not bool((c.attr_idx >= 250).any())
    for training in (False, True):
        ref, terms, dW, dW_terms = ac.bag_reference(c, training)
        out, g = ac.f32_bag(c, training)
        _check(max(ac.ratio(out, ref, terms), ac.ratio(g, dW, dW_terms)), ac.bag_sentinel_margin(c, training))


def test_csr_view_of_the_bags_names_every_bag_once_and_one_twice():
    c = ac.edge_bags(12, seed=12)
    indptr, indices, data, nodes, attr_idx, node_idx, attr_data = ac.bags_as_csr(c)
    assert indices.dtype == torch.int32 and nodes.numel() == len(ac.G_LENS) + 1
    assert sorted(set(nodes.tolist())) == list(range(len(ac.G_LENS))) and nodes.tolist() != sorted(nodes.tolist())
    assert attr_idx.numel() == int((indptr[nodes + 1] - indptr[nodes]).sum()) == node_idx.numel() == attr_data.numel()
