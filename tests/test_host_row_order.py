"""CPU tests of option "row_order" (DESIGN §8): the cost and class definition that row_cost_kernel implements, pinned on a
hand-made graph through its numpy restatement (grand_plus_amd/row_cost.py)."""
import numpy as np

# 8 nodes; degrees 3, 1, 4, 7, 0 (dangling), 8, 1, 2
ROWS = [[1, 2, 3], [0], [0, 1, 3, 4], [0, 1, 2, 4, 5, 6, 7], [], [0, 1, 2, 3, 4, 5, 6, 7], [4], [3, 5]]
INDPTR = np.concatenate([[0], np.cumsum([len(r) for r in ROWS])]).astype(np.int32)
INDICES = np.concatenate([np.array(r, np.int32) for r in ROWS])
SEEDS = np.array([0, 1, 2, 3, 4, 5, 6, 7, -1, 8], np.int32)             # every node, then the two invalid seeds


def test_cost_is_the_edge_count_of_levels_one_and_two():
    """rmax = 0.05: a neighbour u of the seed pushes when 1/d0 >= 0.05 * deg(u).  By hand, c = d0 + the degrees that push:
    seed 0 (1/3): 1 and 2 push (1 + 4), 3 does not (0.35)        -> 3 + 5
    seed 1 (1):   0 pushes (3)                                    -> 1 + 3
    seed 2 (1/4): 0, 1, 4 push (3 + 1 + 0), 3 does not            -> 4 + 4
    seed 3 (1/7): 1, 4, 6, 7 push (1 + 0 + 1 + 2)                 -> 7 + 4
    seed 4: dangling                                              -> 0
    seed 5 (1/8): 1, 4, 6, 7 push                                 -> 8 + 4
    seed 6 (1):   4 pushes nothing (dangling)                     -> 1 + 0
    seed 7 (1/2): 3 and 5 push (7 + 8)                            -> 2 + 15
    and an invalid seed costs 0 without being looked up."""
    from grand_plus_amd.row_cost import cost_class, order_by_class, row_costs
    c = row_costs(INDPTR, INDICES, SEEDS, 0.05, deg_sat=1 << 20)
    assert c.tolist() == [8, 4, 8, 11, 0, 12, 1, 17, 0, 0]
    cls = cost_class(c)
    assert cls.tolist() == [3, 2, 3, 3, 0, 3, 1, 4, 0, 0]                # ilog2(c + 1)
    order = order_by_class(cls)
    assert sorted(order.tolist()) == list(range(len(SEEDS))) and order[0] == 7 and (np.diff(cls[order]) <= 0).all()
    assert set(order[-3:].tolist()) == {4, 8, 9}


def test_a_saturated_degree_counts_as_the_saturation_value():
    """deg_sat = 3: degrees read as 3, 1, 3, 3, 0, 3, 1, 2 -- in the push test and in the sum (an estimate may be off)."""
    from grand_plus_amd.row_cost import row_costs
    c = row_costs(INDPTR, INDICES, SEEDS, 0.05, deg_sat=3)
    # seed 0: all three neighbours now pass (1 + 3 + 3); seed 2: node 3 reads 3 and passes (3 + 1 + 3 + 0); seed 7: 3 + 3;
    # seeds 3 and 5: nodes 0, 2, 3, 5 read 3 and still fail 1/7 and 1/8
    assert c.tolist() == [10, 4, 11, 11, 0, 12, 1, 8, 0, 0]


def test_a_seed_that_fails_its_own_push_test_costs_nothing_and_the_column_cap_scales():
    from grand_plus_amd.row_cost import cost_class, row_costs
    c = row_costs(INDPTR, INDICES, SEEDS, 0.2, deg_sat=1 << 20)          # 1 >= 0.2 * d0 fails for d0 = 7 and 8
    assert c[3] == 0 and c[5] == 0 and c[4] == 0 and c[0] == 3 + 1      # seed 0 (1/3): only node 1 (0.2) passes
    # two columns read of seed 3's seven: node 0 fails, node 1 pushes 1 edge -> 7 + floor(7 * 1 / 2)
    assert row_costs(INDPTR, INDICES, [3], 0.05, deg_sat=1 << 20, cols=2).tolist() == [10]
    assert cost_class([0, 1, 2, 3, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 40]).tolist() == [0, 1, 1, 2, 30, 31, 31]
