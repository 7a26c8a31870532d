"""The evaluation head at its class-count, logit-range and label edges on the GPU: every case of
evaluate_cases.EDGE_DRAWN.  pred, flag, counts and acc are exact; every row's nll is within evaluate_cases.row_bound64,
the bound that follows from eval_head_kernel's order of operations, or is exactly +inf or NaN where torch's float64 is; the
mean is within the mean of the rows' bounds and one rounding.  The largest error over bound per family on the MI355X is
listed in DESIGN §7h; tests/test_host_mutants.py shows on the CPU that these assertions can fail (§7q)."""
import math

import pytest
import torch

import evaluate_cases as ec

pytestmark = pytest.mark.gpu


def _odd(t):
    """The rows that are not finite as numbers that compare: NaN = NaN, +inf = +inf."""
    return torch.nan_to_num(t, nan=1.0)


@pytest.mark.parametrize("name", ec.EDGE_NAMES)
def test_head_at_the_edges(name):
    from grand_plus_amd import eval_head, eval_reduce
    _, z, y, kw = ec.EDGE_DRAWN[ec.EDGE_NAMES.index(name)]
    ref, fam = ec.edge_reference(name), ec.edge_family(name)
    buf = eval_head(z.cuda(), y.cuda(), **{k: v.cuda() for k, v in kw.items()})
    loss, acc, counts = eval_reduce(buf)
    loss, acc = float(loss), float(acc)
    assert torch.equal(buf.pred.cpu().long(), ref["pred"]), name
    assert torch.equal(buf.flag.cpu(), ref["flag"]) and counts.tolist() == ref["counts"], name
    assert acc == ref["acc"], name
    nll, fin = buf.nll.cpu().double(), torch.isfinite(ref["nll"])
    assert torch.equal(torch.isfinite(nll), fin) and torch.equal(_odd(nll[~fin]), _odd(ref["nll"][~fin])), name
    share = float(((nll - ref["nll"]).abs()[fin] / ref["bound"][fin]).max())
    if bool(fin.all()):
        mean, mean_bound = ec.mean_bound64(ref["nll"], ref["bound"])
        print(f"[evaluate] {name}: max row error / bound {share:.3g}, mean error / bound {abs(loss - mean) / mean_bound:.3g}")
        assert share <= 1.0 and abs(loss - mean) <= mean_bound, (name, share, loss, mean)
        torch32 = ec.nll32_on(ref["zz"].cuda(), ref["yy"].cuda())
        if fam in ec.PRINT_ONLY:                              # torch's float32 can be exact there: §7g's rule is printed
            e_t = abs(torch32 - mean)
            print(f"[evaluate] {name}: |ours-ref64| {abs(loss - mean):.3e}  |torch32-ref64| {e_t:.3e}  "
                  f"ratio {abs(loss - mean) / e_t if e_t else float('nan'):.3g} (not asserted)")
        else:
            ec.assert_loss(loss, torch32, mean, name)
    else:
        print(f"[evaluate] {name}: max row error / bound {share:.3g} over the finite rows, mean {loss} (float64: {ref['mean']})")
        assert share <= 1.0, (name, share)
        assert (math.isnan(ref["mean"]) and math.isnan(loss)) or loss == ref["mean"], (name, loss, ref["mean"])


def test_one_class_past_the_limit_is_refused_on_the_device_too(monkeypatch):
    """GP_MAX_CLASSES + 1 classes on the GPU: ValueError, and the native library is not reached."""
    from grand_plus_amd import _native
    from grand_plus_amd.evaluate import eval_head
    z = torch.zeros((2, _native.GP_MAX_CLASSES + 1), device="cuda")
    y = torch.zeros(2, dtype=torch.int64, device="cuda")
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    with pytest.raises(ValueError, match=r"classes must be in \[1, 4096\], got 4097"):
        eval_head(z, y)
