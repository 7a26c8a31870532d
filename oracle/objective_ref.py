"""Plain-PyTorch restatement of the GRAND+ training objective (reference model.py:123-139, 321-331; the same text
in model_mag.py:125-142) -- TEST INFRASTRUCTURE (the checker of tests/test_gpu_objective.py, of the end-to-end steps
in tests/test_gpu_mlp.py and tests/test_gpu_embedding.py, and the timed comparison column of bench_train_step.py and
bench_mlp_step.py), never imported by the product.

Works in the dtype and on the device of its inputs: float64 leaves give the reference gradients through autograd.

Pinned to the reference itself by tests/golden/train_pieces.npz (keys cl_*) and by the step losses of
tests/golden/train_run_*.npz: tests/test_host_reference_training.py.
"""
import torch
import torch.nn.functional as Fn


def consis_loss_ref(logps, tem, conf, kind):
    """consis_loss of model.py:123-139, args.loss = kind."""
    ps = [torch.exp(p) for p in logps]
    sum_p = 0.
    for p in ps:
        sum_p = sum_p + p
    avg_p = sum_p / len(ps)
    sharp_p = (torch.pow(avg_p, 1. / tem) / torch.sum(torch.pow(avg_p, 1. / tem), dim=1, keepdim=True)).detach()
    loss = 0.
    for p in ps:
        if kind == "kl":
            loss += torch.mean((-sharp_p * torch.log(p)).sum(1)[avg_p.max(1)[0] > conf])
        else:
            loss += torch.mean((p - sharp_p).pow(2).sum(1)[avg_p.max(1)[0] > conf])
    return loss / len(ps)


def grand_loss_ref(z, labels, n_l, w, tem, conf, kind, ignore_index=-100):
    """model.py:321-329 on the S logit tensors z[s] (a tensor [S, B, C] or a list; any dtype): (loss, L_sup, L_con)."""
    S = len(z)
    outs, sup = [], 0.
    for s in range(S):
        lp = torch.log_softmax(z[s], dim=-1)
        outs.append(lp[n_l:])
        sup = sup + Fn.nll_loss(lp[:n_l], labels[:n_l], ignore_index=ignore_index)
    sup = sup / S
    con = consis_loss_ref(outs, tem, conf, kind)
    return sup + w * con, sup, con
