"""The fused evaluation tail on the GPU.  Every comparison is against `eval_head` + `eval_reduce` on the same
inputs, bit for bit on all five outputs (nll, pred, flag, the loss/acc pair and the counts; a NaN compares by its bits), with
64 guard elements around every output and the workspace untouched and the ticket counter back at zero after every call."""
import numpy as np
import pytest
import torch

import eval_tail_cases as tc

pytestmark = pytest.mark.gpu

GUARD = 64
NS = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)
CS = (1, 7, 64, 65)


def _bits(t):
    t = t.contiguous()
    return t if t.dtype in (torch.uint8, torch.int64, torch.int32) else t.view(torch.int32)


class Guarded:
    """The outputs of one tail call, each in the middle of a buffer with GUARD elements of a fill value on both sides."""
    FILL = {torch.float32: 7.25, torch.int32: -77, torch.uint8: 0xA5, torch.int64: -77}

    def __init__(self, n, dev):
        self.n = n
        self.full = {name: torch.full((size + 2 * GUARD,), self.FILL[dt], dtype=dt, device=dev)
                     for name, size, dt in (("nll", n, torch.float32), ("pred", n, torch.int32), ("flag", n, torch.uint8),
                                            ("out2", 2, torch.float32), ("counts", 4, torch.int64))}
        ws = torch.full((tc.TAIL_WORKSPACE_BYTES + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        ws[GUARD:GUARD + tc.TAIL_WORKSPACE_BYTES] = 0
        self.full["ws"] = ws

    def mid(self, name):
        t = self.full[name]
        return t[GUARD:t.numel() - GUARD]

    def check(self, what):
        for name, t in self.full.items():
            fill = torch.full((GUARD,), 0xA5 if name == "ws" else self.FILL[t.dtype], dtype=t.dtype, device=t.device)
            assert torch.equal(_bits(t[:GUARD]), _bits(fill)) and torch.equal(_bits(t[-GUARD:]), _bits(fill)), (what, name)
        assert not self.mid("ws").any(), (what, "the ticket counter is back at zero, the padding untouched")


def _pair(z, y, **kw):
    from grand_plus_amd import eval_head, eval_reduce
    buf = eval_head(z, y, **kw)
    loss, acc, counts = eval_reduce(buf)
    return buf, torch.stack([loss, acc]), counts


def _tail(z, y, g=None, **kw):
    """eval_tail into guarded buffers (a fresh set unless given): (EvalBuffers, out2, counts, the Guarded)."""
    from grand_plus_amd import eval_tail
    from grand_plus_amd.evaluate import EvalBuffers
    rows, lrows = kw.get("rows"), kw.get("label_rows")
    n = rows.numel() if rows is not None else lrows.numel() if lrows is not None else z.shape[0]
    g = g or Guarded(n, z.device)
    loss, acc, counts, buf = eval_tail(z, y, out=EvalBuffers(g.mid("nll"), g.mid("pred"), g.mid("flag")), workspace=g.mid("ws"),
                                       result=(g.mid("out2"), g.mid("counts")), **kw)
    assert loss.data_ptr() == g.mid("out2").data_ptr() and acc.data_ptr() == loss.data_ptr() + 4 and loss.dim() == 0
    assert counts.data_ptr() == g.mid("counts").data_ptr() and buf.nll.data_ptr() == g.mid("nll").data_ptr()
    return buf, g.mid("out2"), counts, g


def _assert_same(got, want, what):
    (gb, go, gc), (wb, wo, wc) = got, want
    for name, a, b in (("nll", gb.nll, wb.nll), ("pred", gb.pred, wb.pred), ("flag", gb.flag, wb.flag), ("out", go, wo), ("counts", gc, wc)):
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (what, name)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("n", NS)
def test_the_tail_is_the_head_and_the_reduce_bit_for_bit(n, C):
    z, y = tc.mixed_case(n, C)
    zd, yd = z.cuda(), y.cuda()
    buf, out, counts, g = _tail(zd, yd)
    _assert_same((buf, out, counts), _pair(zd, yd), f"n={n} C={C}")
    g.check(f"n={n} C={C}")
    if n > 4 and C > 1:
        assert set(buf.flag.tolist()) == {tc.WRONG, tc.CORRECT, tc.IGNORED, tc.BAD} or n < 255
    if n == 0:
        assert np.isnan(out.tolist()).all() and counts.tolist() == [0, 0, 0, 0]
    # with both index lists, some of their entries outside the arrays; and with the labels of another length
    R, m = n + 3, n + 5
    z2, y2 = tc.mixed_case(R, C, seed=1, n_labels=m)
    rows, lrows = tc.index_lists(n, R, m)
    z2, y2, rows, lrows = z2.cuda(), y2.cuda(), rows.cuda(), lrows.cuda()
    for kw in (dict(rows=rows, label_rows=lrows), dict(rows=rows), dict(label_rows=lrows)):
        buf, out, counts, g = _tail(z2, y2, **kw)
        _assert_same((buf, out, counts), _pair(z2, y2, **kw), f"n={n} C={C} {sorted(kw)}")
        g.check(f"n={n} C={C} {sorted(kw)}")
        if n > 4 and "rows" in kw and "label_rows" in kw:
            assert buf.pred[0].item() == -1 and buf.flag[[0, 1, 3, 4]].tolist() == [tc.BAD] * 4


def test_the_widest_row_and_all_rows_ignored():
    z, y = tc.mixed_case(5, 4096)
    buf, out, counts, g = _tail(z.cuda(), y.cuda())
    _assert_same((buf, out, counts), _pair(z.cuda(), y.cuda()), "C=4096")
    g.check("C=4096")
    z, y = tc.mixed_case(300, 7)
    y[:] = -100
    buf, out, counts, g = _tail(z.cuda(), y.cuda())
    _assert_same((buf, out, counts), _pair(z.cuda(), y.cuda()), "all ignored")
    assert np.isnan(out[0].item()) and out[1].item() == 0.0 and counts.tolist() == [0, 0, 300, 0]
    g.check("all ignored")


def test_the_cap_and_the_fallback_past_it():
    from grand_plus_amd import _native, eval_tail
    n = tc.TAIL_MAX_ROWS
    z, y = tc.mixed_case(n + 1, 7)
    zd, yd = z.cuda(), y.cuda()
    buf, out, counts, g = _tail(zd[:n], yd[:n])
    _assert_same((buf, out, counts), _pair(zd[:n], yd[:n]), "n=65536")
    g.check("n=65536")
    # one row more: the entry point refuses, the wrapper runs the unfused pair
    g = Guarded(n + 1, zd.device)
    rc = _native.lib().gp_eval_tail(0, zd.data_ptr(), n + 1, 7, None, yd.data_ptr(), n + 1, None, n + 1, -100, g.mid("nll").data_ptr(),
                                    g.mid("pred").data_ptr(), g.mid("flag").data_ptr(), g.mid("ws").data_ptr(), g.mid("out2").data_ptr(),
                                    g.mid("counts").data_ptr(), None)
    assert rc == _native.GP_ERR_INVALID_ARG and "GP_EVAL_TAIL_MAX_ROWS" in _native.lib().gp_last_error().decode()
    torch.cuda.synchronize()
    g.check("refused")
    assert torch.equal(g.mid("out2"), torch.full((2,), 7.25, device="cuda"))    # nothing was written
    buf, out, counts, g = _tail(zd, yd)
    _assert_same((buf, out, counts), _pair(zd, yd), "n=65537")
    g.check("n=65537")
    loss, acc, counts2, _ = eval_tail(zd, yd)                                     # and with everything allocated by the wrapper
    assert torch.equal(_bits(torch.stack([loss, acc])), _bits(out)) and torch.equal(counts2, counts)


def test_the_order_of_the_sum_is_the_mirrors():
    """nll spread over 1e-6 ... 1e3: the tail equals the pair, both are the host mirror's bits from the GPU's own nll, and
    the mirror with the slots summed in the wrong order has another float64 sum on exactly these values."""
    n = tc.SPREAD_N
    z, y = tc.spread_logits(n)
    buf, out, counts, g = _tail(z.cuda(), y.cuda())
    _assert_same((buf, out, counts), _pair(z.cuda(), y.cuda()), "spread")
    g.check("spread")
    nll, flag = buf.nll.cpu().numpy(), buf.flag.cpu().numpy()
    assert nll.min() < 1e-5 and nll.max() > 1e2 and counts.tolist()[0] == n
    right = tc.reduce_mirror(nll, flag)
    got = (np.float32(out[0].item()), np.float32(out[1].item()), counts.tolist())
    print(f"[eval_tail] spread: loss {got[0]!r} mirror {right[0]!r} sum64 {right[3]!r}")
    assert tc.same(got, right, sum64=False)
    assert not tc.same(right, tc.reduce_mirror(nll, flag, "slot_order"))


COUNTER_N = (1025, 3, 2049, 1, 1024)


def _counter_inputs(C=7):
    cases = [tc.mixed_case(n, C, seed=3) for n in COUNTER_N]
    return [(z.cuda(), y.cuda()) for z, y in cases]


def test_five_calls_in_a_row_share_one_workspace():
    inputs = _counter_inputs()
    g = Guarded(max(COUNTER_N), "cuda")
    from grand_plus_amd import eval_tail
    from grand_plus_amd.evaluate import EvalBuffers
    out = EvalBuffers(g.mid("nll"), g.mid("pred"), g.mid("flag"))
    for (z, y), n in zip(inputs, COUNTER_N):
        loss, acc, counts, buf = eval_tail(z, y, out=out, workspace=g.mid("ws"), result=(g.mid("out2"), g.mid("counts")))
        wb, wo, wc = _pair(z, y)
        got = type(wb)(buf.nll[:n], buf.pred[:n], buf.flag[:n])
        _assert_same((got, g.mid("out2"), counts), (wb, wo, wc), f"call n={n}")
        g.check(f"call n={n}")


def test_the_tail_in_a_replayed_graph_on_a_side_stream():
    from grand_plus_amd import eval_tail
    from grand_plus_amd.evaluate import EvalBuffers
    inputs = _counter_inputs()
    g = Guarded(max(COUNTER_N), "cuda")
    out = EvalBuffers(g.mid("nll"), g.mid("pred"), g.mid("flag"))
    res = [(torch.empty(2, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda")) for _ in COUNTER_N]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                 # eager on a side stream first: it loads the code
        for (z, y), r in zip(inputs, res):
            eval_tail(z, y, out=out, workspace=g.mid("ws"), result=r)
    side.synchronize()
    for (z, y), n, r in zip(inputs, COUNTER_N, res):
        _, wo, wc = _pair(z, y)
        assert torch.equal(_bits(r[0]), _bits(wo)) and torch.equal(r[1], wc), f"side stream n={n}"
    g.check("side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                 # five tails in a row, one workspace
        for (z, y), r in zip(inputs, res):
            eval_tail(z, y, out=out, workspace=g.mid("ws"), result=r)
    for replay in range(3):
        for i, (z, y) in enumerate(inputs):                                       # the logits rewritten in place in between
            z2, _ = tc.mixed_case(z.shape[0], z.shape[1], seed=10 + replay)
            z.copy_(z2)
        for r in res:
            r[0].fill_(-1.0)
            r[1].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for (z, y), n, r in zip(inputs, COUNTER_N, res):
            wb, wo, wc = _pair(z, y)
            assert torch.equal(_bits(r[0]), _bits(wo)) and torch.equal(r[1], wc), f"replay {replay} n={n}"
        wb, _, _ = _pair(*inputs[-1])                                             # the buffers hold the last call's rows
        n = COUNTER_N[-1]
        _assert_same((EvalBuffers(out.nll[:n], out.pred[:n], out.flag[:n]), res[-1][0], res[-1][1]), (wb, res[-1][0], res[-1][1]), "rows")
        g.check(f"replay {replay}")
