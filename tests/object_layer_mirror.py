"""Float64 CPU statement of the label loss and its gradient (csrc/labels.hip) in plain torch, and the confusion matrix in numpy.
Test infrastructure: nothing under monogs_amd/ imports it.

    counted(p)   = (valid is None or valid[p] != 0) and labels[p] < K,   N = number of counted pixels
    L            = (1 / N) sum over counted p of [ logsumexp_k feat[k, p] - feat[labels[p], p] ]
    d_feat[k, p] = (softmax_k(feat[:, p]) - [k == labels[p]]) / N on counted pixels, 0 elsewhere;  N == 0: L = 0, d_feat = 0
"""
import numpy as np
import torch


def counted_mask(labels, valid, K):
    labels = torch.as_tensor(labels).cpu().long()
    on = labels < K
    if valid is not None:
        on &= torch.as_tensor(valid).cpu() != 0
    return on


def label_loss_mirror(feat, labels, valid=None):
    """``(L, d_feat, N)`` in float64 from ``feat [K, H, W]`` (any float dtype; converted exactly), ``labels [H, W]`` integer and
    ``valid [H, W]`` or None."""
    x = feat.detach().cpu().double()
    K = x.shape[0]
    labels = torch.as_tensor(labels).cpu().long()
    on = counted_mask(labels, valid, K)
    N = int(on.sum())
    d = torch.zeros_like(x)
    if N == 0:
        return torch.zeros((), dtype=torch.float64), d, 0
    safe = torch.where(on, labels, torch.zeros_like(labels))
    lse = torch.logsumexp(x, dim=0)
    picked = torch.gather(x, 0, safe[None])[0]
    L = ((lse - picked) * on).sum() / N
    soft = torch.exp(x - lse[None])
    onehot = torch.zeros_like(x).scatter_(0, safe[None], 1.0)
    d = (soft - onehot) * on[None] / N
    return L, d, N


def confusion_mirror(pred, gt, valid, K):
    """``(counts [K, K] indexed [gt, pred], side [2])`` with numpy's ``bincount``: ``side = {counted pixels whose prediction lies
    outside 0..K-1 (-1 = not seen), pixels not counted}``."""
    pred = np.asarray(torch.as_tensor(pred).cpu()).astype(np.int64).reshape(-1)
    gt = np.asarray(torch.as_tensor(gt).cpu()).astype(np.int64).reshape(-1)
    on = gt < K
    if valid is not None:
        on &= np.asarray(torch.as_tensor(valid).cpu()).reshape(-1) != 0
    seen = (pred >= 0) & (pred < K)
    both = on & seen
    counts = np.bincount(gt[both] * K + pred[both], minlength=K * K).reshape(K, K)
    return counts.astype(np.int64), np.array([int((on & ~seen).sum()), int((~on).sum())], dtype=np.int64)
