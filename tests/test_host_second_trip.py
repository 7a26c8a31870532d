"""CPU tests of the second-trip cases (tests/second_trip_cases.py).  No mutated kernel is ever run, so that
the GPU tests of tests/test_gpu_second_trip.py bite rests on what is shown here: every grid cap is read out of the sources
and equals what the cases were sized for; every case is past its cap, and the index range of its second trip is the one
the GPU test looks at on its own; and every exact reference is exact -- each destination's terms are whole quanta whose
absolute sum stays below 2^24, and on 10 000 entries a float32 left-to-right loop gives the bincount's bits."""
import numpy as np
import pytest

import mag_det_cases as dc
import optim_cases as oc
import second_trip_cases as st

f32 = np.float32


def _left_to_right(dest, terms, n_dest):
    """float32 accumulation entry after entry, from 0.0f: what a sequential kernel computes."""
    acc = np.zeros(n_dest, f32)
    for a, x in zip(dest.tolist(), terms.astype(f32)):
        acc[a] = f32(acc[a] + x)
    return acc


def _assert_exact(keys, sorted_keys, terms, n_dest, quantum, want):
    """The exactness precondition over the whole case, then the loop over the last 10 000 sorted entries: they hold the
    whole segments of the second trip's own destinations."""
    margin = st.exact_margin(keys, terms, n_dest, quantum)
    per_dest = np.bincount(keys, minlength=n_dest)
    print(f"largest sum of |terms| of a destination: {margin:.0f} quanta; most contributions {int(per_dest.max())}")
    assert margin < 2 ** 24 and per_dest.max() <= 2 ** 12
    assert np.array_equal(np.bincount(keys, weights=terms, minlength=n_dest).astype(f32), want.numpy().reshape(-1))
    order = np.argsort(keys, kind="stable")[-10_000:]
    loop = _left_to_right(keys[order], terms[order], n_dest)
    ref = np.bincount(keys[order], weights=terms[order], minlength=n_dest).astype(f32)
    assert np.array_equal(loop.view(np.int32), ref.view(np.int32))
    whole = st.second_trip_only(sorted_keys, n_dest, len(keys) - 10_000)
    assert whole.any() and np.array_equal(loop[whole].view(np.int32), want.numpy().reshape(-1)[whole].view(np.int32))


def _assert_second_trip_rows(sorted_keys, n_dest, want):
    """Some destinations lie wholly in the windows past the gather's first trip, and their reference is not zero."""
    only = st.second_trip_only(sorted_keys, n_dest)
    assert only.sum() >= 2 and bool((want.numpy().reshape(-1)[only] != 0).all()), only.sum()
    assert sorted_keys[st.GATHER_ONE_TRIP - 1] <= np.flatnonzero(only)[0] - 1        # the first trip never reaches them


def test_every_cap_in_the_sources_is_the_one_the_cases_were_sized_for():
    assert st.source_caps() == st.CAPS
    assert oc.CHUNK == st.CAPS["optim_chunk"] and oc.GRID_CAP == st.CAPS["optim_grid"]
    assert st.GATHER_ONE_TRIP == 4_194_240 and st.MAG_LEN_ONE_TRIP == 2_097_152 and st.MAG_KEYS_ONE_TRIP == 32_768
    assert st.BAG_DEN_ONE_TRIP == st.HEAD_ONE_TRIP == 262_140 and st.STEP_ONE_TRIP == st.FIT_ONE_TRIP == 1_048_576


def test_the_mag_case_passes_five_caps_and_its_reference_is_exact():
    c = st.mag_case()
    n_slots = st.MAG_B * st.MAG_K
    assert st.MAG_LEN_ONE_TRIP < n_slots < 1.002 * st.MAG_LEN_ONE_TRIP             # mag_slot_len_kernel: just above
    assert n_slots > st.MAG_KEYS_ONE_TRIP                                          # mag_keys_kernel's slot loop
    assert st.MAG_B > st.MAG_ROWS_ONE_TRIP                                         # mag_slot_grad_kernel and the atomic backward
    assert st.GATHER_ONE_TRIP < c["total"] < 1.001 * st.GATHER_ONE_TRIP            # gather_sum_kernel<MagOp>
    assert set(np.unique(c["slot_len"]).tolist()) == {0, 1, 2} and c["slot_base"][-1] == c["total"] == len(c["keys"])
    assert 0 <= c["keys"].min() and c["keys"].max() < st.MAG_V
    # second trips by index: slots from 2 097 152 (a thread each) and from 32 768 (a wave each), batch rows from 8 192,
    # sorted positions from 4 194 240; all of them hold live work
    assert c["slot_len"][st.MAG_LEN_ONE_TRIP:].sum() > 0 and c["G"][st.MAG_ROWS_ONE_TRIP:].abs().sum() > 0
    _assert_second_trip_rows(c["sorted_keys"], st.MAG_V, c["dW"])
    _assert_exact(c["keys"], c["sorted_keys"], c["terms"], st.MAG_V, st.MAG_QUANTUM, c["dW"])


def test_the_small_tail_case_takes_four_passes_of_one_workgroup():
    assert dc.SLACK[-1] == 1000 and dc.GRID[1] == (1, 1)
    threads = st.BLOCK * 1                                                         # one slot: one workgroup of 256 threads
    assert -(-dc.SLACK[-1] // threads) == 4 and max(dc.SLACK[:-1]) < threads       # the other slacks never left the first pass


def test_the_rows_case_passes_both_caps_and_its_reference_is_exact():
    c = st.rows_case()
    assert st.ROWS_B > st.ROWS_DEN_ONE_TRIP                                        # rows_inv_den_kernel: 41 rows on the second trip
    assert st.ROWS_B * st.ROWS_K == len(c["keys"]) == 4_196_864 > st.GATHER_ONE_TRIP   # gather_sum_kernel<RowsOp>
    assert st.ROWS_K * st.ROWS_QUANTUM == 1.0                                      # the row denominator
    assert c["G"][st.ROWS_DEN_ONE_TRIP:].abs().sum() > 0
    _assert_second_trip_rows(c["sorted_keys"], st.ROWS_N, c["grad"])
    _assert_exact(c["keys"], c["sorted_keys"], c["terms"], st.ROWS_N, st.ROWS_QUANTUM, c["grad"])


def test_the_bag_case_passes_both_caps_and_its_reference_is_exact():
    c = st.bag_case()
    assert st.BAG_M > st.BAG_DEN_ONE_TRIP                                          # bag_inv_den_kernel: 41 bags on the second trip
    assert st.BAG_M * st.BAG_LEN == len(c["keys"]) == 4_194_896 > st.GATHER_ONE_TRIP   # gather_sum_kernel<BagOp>
    assert st.BAG_LEN * st.BAG_QUANTUM == 1.0                                      # the bag denominator
    assert c["G"][st.BAG_DEN_ONE_TRIP:].abs().sum() > 0
    _assert_second_trip_rows(c["sorted_keys"], st.BAG_V, c["dW"])
    _assert_exact(c["keys"], c["sorted_keys"], c["terms"], st.BAG_V, st.BAG_QUANTUM, c["dW"])


def test_the_optimiser_sets_pass_the_grid_and_the_second_group_is_the_larger():
    ends, total, second = st.stride_chunks()
    assert ends == [1, 1027, 1028] and total == 1028 > st.OPTIM_ONE_TRIP
    # workgroups 0 .. 3 on their second trip: two whole chunks, the 5-element tail, the whole third tensor
    assert second == [(1, 1023 * 4096, 4096), (1, 1024 * 4096, 4096), (1, 1025 * 4096, 5), (2, 0, 7)]
    assert oc.OWN_TESTS == ("stride", "solo") and oc.STRIDE_STEPS == 2
    late = [oc.numel(s) for s in oc.SETS["late_big"]]
    chunks = [sum(-(-n // oc.CHUNK) for n in late[:oc.MAX_TENSORS]), sum(-(-n // oc.CHUNK) for n in late[oc.MAX_TENSORS:])]
    assert len(late) == oc.MAX_TENSORS + 2 and chunks == [32, 42] and max(chunks) < st.OPTIM_ONE_TRIP
    assert oc.SETS["solo"] == [(1,)]
    assert oc.SEED_ORDER[:5] == tuple(sorted(oc.SEED_ORDER[:5]))                   # the older sets keep the inputs they had


def test_the_mask_case_puts_the_segment_boundary_on_the_second_trip():
    assert st.MASK_ROW_ITEMS == 1_049_600 and st.STEP_ONE_TRIP < st.MASK_ROW_ITEMS < st.MASK_ITEMS < 2 * st.STEP_ONE_TRIP
    filled, rows = st.mask_case()
    assert st.MASK_ROWS >= st.MASK_B == rows.numel() == len(set(rows.tolist())) and filled.numel() == st.MASK_ROWS
    assert int(filled.min()) == 0 and int(filled.max()) == st.MASK_K and 0 < int((filled[rows.long()] < st.MASK_K).sum())


def test_the_fit_cases_pass_the_grid_and_the_probes_straddle_it():
    assert st.SELECT_TOTAL == 1_048_879 > st.FIT_ONE_TRIP
    p = st.SELECT_PROBES
    assert len(p) == 256 and len(set(p.tolist())) == 256 and p.min() == st.SELECT_TRAIN and p.max() == st.SELECT_TOTAL - 1
    assert ((p >= st.FIT_ONE_TRIP - 64) & (p < st.FIT_ONE_TRIP)).sum() == 64 and (p >= st.FIT_ONE_TRIP).sum() == 128
    w = st.SNAPSHOT_WORDS
    assert w[0] + w[1] > st.FIT_ONE_TRIP > w[0] and sum(w) < 2 * st.FIT_ONE_TRIP   # tensor 3 starts on the second trip


@pytest.mark.parametrize("C", st.HEAD_C)
def test_the_head_case_leaves_37_rows_of_every_kind_to_the_second_trip(C):
    z, y, y_valid = st.head_case(C)
    assert st.HEAD_N - st.HEAD_ONE_TRIP == 37 and z.shape == (st.HEAD_N, C)
    tail = y[st.HEAD_ONE_TRIP:]
    assert bool((tail == st.HEAD_IGNORE).any()) and bool((tail >= C).any()) and bool((tail == -1).any())
    assert int(((tail >= 0) & (tail < C)).sum()) >= 30
    assert int((y == st.HEAD_IGNORE).sum()) > 2000 and int((y >= C).sum()) > 1000 and int((y == -1).sum()) > 1000
    assert bool(((y_valid == y) | (y_valid == st.HEAD_IGNORE)).all()) and int((y_valid != y).sum()) == int(((y >= C) | (y == -1)).sum())
