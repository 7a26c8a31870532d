#!/usr/bin/env python3
"""bench_mag_step.py -- MAG's data path around the precompute, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  Cases:
  mag-train    B = 40 rows (20 labelled + 20 unlabelled, run_mag.sh), K = 32, H = 64, --sample 2:
               embedding_bag_csr + random_prop, forward and backward (model_mag.py:339-361 without the MLP)
  mag-valid    B = 100 (valid's batch size, model_mag.py:145), forward only
  predict-emb  10 000-node batches of predict's emb pass (model_mag.py:197-205), forward only
Per case: time of this project's path (CUDA events around the whole step, launches included), algorithmic
bytes and the fraction of 8 TB/s; for the backward also the atomic bytes (nnz * H * 4) and their fraction of
1.3 TB/s.  Comparison columns: the same formulation in plain torch (F.embedding + dropout + index_add_) on the
same GPU, fed with device-resident COO tensors; and the reference's host preparation (topk_adj[batch],
.nonzero(), features[neighbor_idx], .nonzero(), upload) timed with scipy on a synthetic CSR.

The MAG vocabulary size and bag lengths are not known here: --vocab, --bag and --nodes are ASSUMPTIONS
(defaults: 500 000 attribute ids, 20 attributes per node, 2 000 000 nodes), as are the synthetic [S x K] rows.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

from _bench_steps import emit, synthetic_rows, timed, torch_prop  # noqa: E402
from grand_plus_amd.augment import algorithmic_bytes, random_prop  # noqa: E402
from grand_plus_amd.embedding import embedding_bag_csr, flatten_rows  # noqa: E402

HBM, ATOMIC = 8.0e12, 1.3e12


def torch_emb(W, attr_idx, node_idx, attr_data, p, training, n_out):
    fe = Fn.dropout(Fn.embedding(attr_idx, W), p, training=training)
    num = torch.zeros((n_out, W.shape[1]), device=W.device).index_add_(0, node_idx, fe * attr_data[:, None])
    den = torch.zeros((n_out, 1), device=W.device).index_add_(0, node_idx, attr_data[:, None])
    return num / (den + 1e-10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2_000_000)
    ap.add_argument("--vocab", type=int, default=500_000)
    ap.add_argument("--bag", type=int, default=20, help="attributes per node (each node gets 1 .. 2*bag-1, mean bag)")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-host", action="store_true", help="skip the scipy host-preparation column")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    N, V, H, K = a.nodes, a.vocab, a.hidden, a.K
    lens = rng.integers(1, 2 * a.bag, N)
    indptr = np.zeros(N + 1, np.int64); np.cumsum(lens, out=indptr[1:])
    indices = rng.integers(0, V, int(indptr[-1])).astype(np.int32)
    data = (rng.random(int(indptr[-1]), dtype=np.float32) + 0.05).astype(np.float32)
    ip, ix, dt = (torch.from_numpy(x).to(dev) for x in (indptr, indices, data))
    W = (torch.randn((V, H), device=dev) * 0.1).requires_grad_(True)
    S = 20_000                                                                   # resident [S x K] rows (synthetic)
    col, val, filled = synthetic_rows(rng, dev, S, K, N)
    host = None
    if not a.no_host:
        import scipy.sparse as sp
        features = sp.csr_matrix((data, indices, indptr), shape=(N, V))
        topk_adj = sp.csr_matrix((val.cpu().numpy(), col.cpu().numpy(), np.arange(0, S * K + 1, K)), shape=(S, N))
        host = (features, topk_adj)

    def host_prep_us(batch):
        features, topk_adj = host
        reps = []
        for _ in range(5):
            t0 = time.perf_counter()
            sub = topk_adj[batch]                                                # model_mag.py:337
            source_idx, neighbor_idx = sub.nonzero()                             # :339
            batch_feat = features[neighbor_idx]                                  # :341
            node_idx, attr_idx = batch_feat.nonzero()                            # :345
            for arr, dtp in ((sub.data, torch.float32), (source_idx, torch.long), (batch_feat.data, torch.float32), (node_idx, torch.long)):
                torch.tensor(arr, dtype=dtp).to(dev)
            torch.cuda.synchronize()
            reps.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(reps))

    for name, B, train in (("mag-train", 40, True), ("mag-valid", 100, False), ("predict-emb", 10_000, False)):
        rows = torch.from_numpy(rng.choice(S, B, replace=False).astype(np.int32)).to(dev) if name != "predict-emb" else None
        if rows is not None:
            nbr, scores, mat_idx = flatten_rows(col, val, filled, K, rows)
        else:
            nbr = torch.arange(0, B, dtype=torch.int64, device=dev)
        M = nbr.numel()
        blens = ip[nbr + 1] - ip[nbr]
        nnz = int(blens.sum())
        # device COO for the plain-torch formulation (what the reference's tensors are after the upload)
        node_idx = torch.repeat_interleave(torch.arange(M, device=dev), blens)
        starts = torch.repeat_interleave(ip[nbr] - (torch.cumsum(blens, 0) - blens), blens)
        pos = torch.arange(nnz, device=dev) + starts
        attr_idx, attr_data = ix[pos].long(), dt[pos]

        if name == "mag-train":
            def ours():
                loss = 0.
                for _ in range(2):                                               # --sample 2
                    emb = embedding_bag_csr(W, ip, ix, dt, nodes=nbr, input_droprate=0.5, training=True, validate=False)
                    loss = loss + random_prop(emb, scores, mat_idx, 0.5, training=True).sum()
                loss.backward()

            def plain():
                loss = 0.
                for _ in range(2):
                    emb = torch_emb(W, attr_idx, node_idx, attr_data, 0.5, True, M)
                    loss = loss + torch_prop(emb, scores, mat_idx, 0.5, True, B).sum()
                loss.backward()
            passes = 2
        else:
            def ours():
                with torch.no_grad():
                    emb = embedding_bag_csr(W, ip, ix, dt, nodes=nbr, training=False, validate=False)
                    if rows is not None:
                        random_prop(emb, scores, mat_idx, 0.5, training=False)

            def plain():
                with torch.no_grad():
                    emb = torch_emb(W, attr_idx, node_idx, attr_data, 0.0, False, M)
                    if rows is not None:
                        torch_prop(emb, scores, mat_idx, 0.5, False, B)
            passes = 1
        us = timed(ours, a.iters, 1, warmup=3)[0]
        us_plain = timed(plain, a.iters, 1, warmup=3)[0]
        W.grad = None
        emb_bytes = nnz * (4 * H + 8) + M * 4 * H                                # table rows + (id, weight) + output rows
        prop_bytes = algorithmic_bytes(M, B, H) if rows is not None else 0
        fwd_bytes = passes * (emb_bytes + prop_bytes)
        rec = {"case": name, "B": B, "K": K, "H": H, "rows_M": M, "attr_nnz": nnz, "sample": passes,
               "assumed_vocab": V, "assumed_bag_mean": a.bag, "assumed_nodes": N,
               "ours_us": round(us, 1), "torch_formulation_us": round(us_plain, 1),
               "speedup_vs_torch": round(us_plain / us, 2), "fwd_alg_bytes": fwd_bytes}
        if train:
            atomic = passes * nnz * H * 4                                         # dW adds (budget of §1d)
            bwd_bytes = passes * (M * H * 4 + M * H * 4) + atomic                 # grad_out reads + grad_feats writes + atomics
            rec.update({"bwd_atomic_bytes": atomic, "alg_bytes": fwd_bytes + bwd_bytes,
                        "frac_of_8TBps": round((fwd_bytes + bwd_bytes) / (us * 1e-6) / HBM, 5),
                        "atomic_frac_of_1.3TBps_at_step_time": round(atomic / (us * 1e-6) / ATOMIC, 5)})
        else:
            rec.update({"alg_bytes": fwd_bytes, "frac_of_8TBps": round(fwd_bytes / (us * 1e-6) / HBM, 5)})
        if host is not None:
            batch = rows.cpu().numpy() if rows is not None else None
            if batch is not None:
                rec["reference_host_prep_us"] = round(host_prep_us(batch), 1)
            else:
                features = host[0]
                t0 = time.perf_counter()
                bf = features[0:B]; n_i, a_i = bf.nonzero()
                torch.tensor(bf.data, dtype=torch.float32).to(dev); torch.tensor(n_i, dtype=torch.long).to(dev)
                torch.cuda.synchronize()
                rec["reference_host_prep_us"] = round((time.perf_counter() - t0) * 1e6, 1)
        emit(rec)


if __name__ == "__main__":
    main()
