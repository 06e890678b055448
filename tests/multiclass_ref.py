"""The formulas of unet_zoo_amd.MulticlassLoss restated with torch in float64 on the CPU: the reference of
tests/test_multiclass_loss_gpu.py, pinned against F.cross_entropy, RegionLoss's documented soft Dice and a hand-computed case
in tests/test_multiclass_loss.py.  Nothing here touches the library."""
import torch

DEFAULTS = dict(w_ce=1.0, w_dice=1.0, smooth=1.0, label_smoothing=0.0, class_weight=None, ignore_index=-100,
                include_background=True, reduce="image", square=False)


def settings(**kw):
    s = dict(DEFAULTS)
    s.update(kw)
    return s


def ce_dice_settings(w_ce=0.4, w_dice=0.6):
    """what MulticlassLoss.ce_dice() must build"""
    return settings(w_ce=w_ce, w_dice=w_dice, square=True, smooth=1e-5, reduce="batch")


def _flat(x, y):
    """x (N, K, ...) -> (N, K, HW) in `x`'s dtype, y (N, ...) or (N, 1, ...) -> (N, HW) int64"""
    N, K = x.shape[0], x.shape[1]
    return x.reshape(N, K, -1), y.reshape(N, -1).long()


def valid_mask(y, K, ignore_index):
    return (y != ignore_index) & (y >= 0) & (y < K)


def ce_part(x, y, class_weight=None, ignore_index=-100, label_smoothing=0.0):
    """sum_valid sum_c a_c (-log p_c) / sum_valid w_y with a_c = (1 - e) w_c [c == y] + (e / K) w_c; 0 when no pixel is valid"""
    x, y = _flat(x.double(), y)
    K = x.shape[1]
    w = torch.ones(K, dtype=torch.float64) if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float64)
    v = valid_mask(y, K, ignore_index)
    logp = torch.log_softmax(x, dim=1)                                  # (N, K, HW)
    onehot = torch.nn.functional.one_hot(torch.where(v, y, torch.zeros_like(y)), K).permute(0, 2, 1).double()
    a = ((1.0 - label_smoothing) * onehot + label_smoothing / K) * w.view(1, K, 1)
    num = (-(a * logp).sum(1) * v).sum()
    den = (w[torch.where(v, y, torch.zeros_like(y))] * v).sum()
    if den.item() == 0.0:
        return num * 0.0
    return num / den


def dice_part(x, y, smooth=1.0, ignore_index=-100, include_background=True, reduce="image", square=False):
    """mean over groups and classes of C of 1 - (2 I + smooth) / (S + T + smooth), sums over valid pixels"""
    x, y = _flat(x.double(), y)
    N, K = x.shape[0], x.shape[1]
    v = valid_mask(y, K, ignore_index)
    p = torch.softmax(x, dim=1) * v.unsqueeze(1)
    onehot = torch.nn.functional.one_hot(torch.where(v, y, torch.zeros_like(y)), K).permute(0, 2, 1).double() * v.unsqueeze(1)
    I = (p * onehot).sum(2)                                             # (N, K)
    S = (p * p if square else p).sum(2)
    T = onehot.sum(2)
    if reduce == "batch":
        I, S, T = I.sum(0, keepdim=True), S.sum(0, keepdim=True), T.sum(0, keepdim=True)
    elif reduce != "image":
        raise ValueError(reduce)
    term = 1.0 - (2.0 * I + smooth) / (S + T + smooth)
    if not include_background:
        term = term[:, 1:]
    return term.mean()


def loss_map(x, y, **kw):
    """w_ce CE + w_dice dice of one map (float64; differentiable with respect to x)"""
    s = settings(**kw)
    loss = 0.0
    if s["w_ce"] != 0:
        loss = loss + s["w_ce"] * ce_part(x, y, s["class_weight"], s["ignore_index"], s["label_smoothing"])
    if s["w_dice"] != 0:
        loss = loss + s["w_dice"] * dice_part(x, y, s["smooth"], s["ignore_index"], s["include_background"], s["reduce"],
                                              s["square"])
    return loss


def reference(maps, y, weights, **kw):
    """(loss, [d loss / d map]) of sum_m weights[m] * loss_map(maps[m]) in float64"""
    leaves = [m.detach().double().requires_grad_(True) for m in maps]
    loss = sum(w * loss_map(v, y, **kw) for w, v in zip(weights, leaves))
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return loss.detach(), [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]


def metric_and_counts(x, y, ignore_index=-100, include_background=True):
    """(metric, counts): prediction argmax_K x (ties: the lowest index); over the valid pixels of the batch TP_c, P_c, T_c;
    the metric is the mean of 2 TP_c / (P_c + T_c) over the classes of C with P_c + T_c > 0, 1 when there is none; counts is
    (K + 1, 3) int64: TP, P, T per class, then (valid, ignored, out of range).  Integer arithmetic: exact."""
    xf, yf = _flat(x.double(), y)
    K = xf.shape[1]
    v = valid_mask(yf, K, ignore_index)
    pred = xf.argmax(dim=1)                                             # the first maximum, as torch.argmax documents
    counts = torch.zeros(K + 1, 3, dtype=torch.int64)
    vals = []
    for c in range(K):
        tp = int(((pred == c) & (yf == c) & v).sum())
        pc = int(((pred == c) & v).sum())
        tc = int(((yf == c) & v).sum())
        counts[c] = torch.tensor([tp, pc, tc])
        if (include_background or c > 0) and pc + tc > 0:
            vals.append(2.0 * tp / (pc + tc))
    ign = int((yf == ignore_index).sum())
    counts[K] = torch.tensor([int(v.sum()), ign, yf.numel() - int(v.sum()) - ign])
    return (sum(vals) / len(vals) if vals else 1.0), counts
