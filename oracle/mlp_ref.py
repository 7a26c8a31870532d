"""Plain-PyTorch restatement of the reference's two MLPs, constructor and forward (model.py:48-66 and
model_mag.py:57-67), with F.batch_norm and dropout by explicit keep masks -- TEST INFRASTRUCTURE (the checker of
tests/test_gpu_mlp.py), never imported by the product.

The submodule names are the reference's, so a state_dict moves between these and grand_plus_amd.mlp's modules.
forward(X, keeps) takes one sample, as the reference calls it once per sample; keeps[i] is layer i's 0/1 mask (unused
in eval mode).  `last_a` is the input of the last Linear, which the tests scale their output tolerance by.

Pinned to the reference itself by tests/golden/train_pieces.npz (keys mlp_*) and tests/golden/train_mag.npz:
tests/test_host_reference_training.py.
"""
import torch
import torch.nn as nn
import torch.nn.functional as Fn


def _normalize(x):
    return x / (1e-12 + torch.norm(x, p=2, dim=-1, keepdim=True))


def _drop(x, p, keep):
    if keep is None or p == 0:
        return x
    return x * keep.to(x.dtype) / (1.0 - p) if p < 1 else x * 0.0


def _bn(bn, x, training):
    return Fn.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, training, bn.momentum, bn.eps)


class RefMLP(nn.Module):
    """model.py's MLP (constructor and forward), dropout by explicit masks."""

    def __init__(self, num_features, num_classes, hidden_size, nlayers, use_bn, input_dropout, hidden_dropout, node_norm):
        super().__init__()
        if nlayers == 1:
            fcs, bns = [nn.Linear(num_features, num_classes)], [nn.BatchNorm1d(num_features)]
        else:
            fcs, bns = [nn.Linear(num_features, hidden_size)], [nn.BatchNorm1d(num_features)]
            for _ in range(nlayers - 2):
                fcs.append(nn.Linear(hidden_size, hidden_size))
                bns.append(nn.BatchNorm1d(hidden_size))
            bns.append(nn.BatchNorm1d(hidden_size))
            fcs.append(nn.Linear(hidden_size, num_classes))
        self.fcs, self.bns = nn.ModuleList(fcs), nn.ModuleList(bns)
        self.input_droprate, self.hidden_droprate = input_dropout, hidden_dropout
        self.use_bn, self.node_norm = use_bn, node_norm

    def forward(self, X, keeps):
        if self.node_norm:
            X = _normalize(X).detach()
        if self.use_bn:
            X = _bn(self.bns[0], X, self.training)
        embs = _drop(X, self.input_droprate, keeps[0] if self.training else None)
        self.last_a = embs
        embs = self.fcs[0](embs)
        for i, (fc, bn) in enumerate(zip(self.fcs[1:], self.bns[1:])):
            embs = Fn.relu(embs)
            if self.node_norm:
                embs = _normalize(embs)
            if self.use_bn:
                embs = _bn(bn, embs, self.training)
            embs = _drop(embs, self.hidden_droprate, keeps[i + 1] if self.training else None)
            self.last_a = embs
            embs = fc(embs)
        return embs


class RefMagMLP(nn.Module):
    """model_mag.py's MLP (constructor and forward)."""

    def __init__(self, num_features, num_classes, hidden_size, nlayers, use_bn, input_dropout, hidden_dropout, node_norm):
        super().__init__()
        if nlayers == 1:
            self.embeds = nn.Embedding(num_features, num_classes)
            self.fcs, self.bns = nn.ModuleList([]), nn.ModuleList([])
        else:
            self.embeds = nn.Embedding(num_features, hidden_size)
            fcs, bns = [], []
            for _ in range(nlayers - 2):
                fcs.append(nn.Linear(hidden_size, hidden_size))
                bns.append(nn.BatchNorm1d(hidden_size))
            bns.append(nn.BatchNorm1d(hidden_size))
            fcs.append(nn.Linear(hidden_size, num_classes))
            self.fcs, self.bns = nn.ModuleList(fcs), nn.ModuleList(bns)
        self.input_droprate, self.hidden_droprate = input_dropout, hidden_dropout
        self.use_bn, self.node_norm = use_bn, node_norm

    def forward(self, X, keeps):
        embs = X
        for i, (fc, bn) in enumerate(zip(self.fcs, self.bns)):
            embs = Fn.relu(embs)
            if self.node_norm:
                embs = _normalize(embs)
            if self.use_bn:
                embs = _bn(bn, embs, self.training)
            embs = _drop(embs, self.hidden_droprate, keeps[i] if self.training else None)
            self.last_a = embs
            embs = fc(embs)
        return embs
