"""The counts, histograms, scores and curves of unet_zoo_amd.ConfusionMetrics restated in numpy: what the GPU tests compare
against.  Counts and histograms come from integer operations (searchsorted(side="right"), bincount); scores and curves are
float64.  Shares no code with unet_zoo_amd/confusion.py; the curve definitions are pinned against brute-force counts by
tests/test_confusion_metrics.py.

Binary mode, per (image, channel) plane: prediction x > 0, target t > 0.5 (x = 0, t = 0.5 and a NaN logit are negative);
    counts = TP, FP, FN, TN;  hist[s, b] = #{(t > 0.5) == s and bin(x) == b},  bin(x) = #{k : x >= e_k}, NaN in bin 0
Class mode, per image: prediction argmax_K with ties to the lowest index; a pixel whose label is ignore_index or outside [0, K)
is counted nowhere;  counts[t, p] = #{label == t and prediction == p};  pairs are the classes first_class .. K - 1
Scores of a pair: dice = 2 TP / (2 TP + FP + FN), iou = TP / (TP + FP + FN), precision = TP / (TP + FP), recall = TP / (TP + FN),
specificity = TN / (TN + FP); 0 where the denominator is 0, except dice = iou = 1 when prediction and target are both empty;
state = 0 both non-empty, 1 prediction empty, 2 target empty, 3 both empty
"""
import numpy as np


def edges_uniform(B: int) -> np.ndarray:
    """float32(log(k / (B - k))), k = 1 .. B - 1, formed in float64"""
    return np.array([np.log(np.float64(k) / np.float64(B - k)) for k in range(1, B)], dtype=np.float64).astype(np.float32)


def edges_of(probabilities) -> np.ndarray:
    p = np.asarray(probabilities, dtype=np.float64)
    return (np.log(p) - np.log1p(-p)).astype(np.float32)


def bins_of(x: np.ndarray, edges: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    b = np.searchsorted(np.asarray(edges, dtype=np.float32), x, side="right")
    return np.where(np.isnan(x), 0, b).astype(np.int64)      # numpy sorts a NaN above everything; the kernel's x >= e is false


def score_row(tp: int, fp: int, fn: int, tn: int):
    """(dice, iou, precision, recall, specificity) in float64 and the state"""
    tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)
    state = (1 if tp + fp == 0 else 0) | (2 if tp + fn == 0 else 0)

    def ratio(num, den):
        return float(np.float64(num) / np.float64(den)) if den > 0 else 0.0
    dice, iou = ratio(2 * tp, 2 * tp + fp + fn), ratio(tp, tp + fp + fn)
    if state == 3:
        dice = iou = 1.0
    return (dice, iou, ratio(tp, tp + fp), ratio(tp, tp + fn), ratio(tn, tn + fp)), state


def binary(logits: np.ndarray, target: np.ndarray, edges: np.ndarray):
    """(counts (N, C, 4) int64, hist (N, C, 2, B) int64, out (N, C, 5) float64, state (N, C) int64) of (N, C, H, W) float32
    logits against (N, C, H, W) float32 maps"""
    logits, target = np.asarray(logits, dtype=np.float32), np.asarray(target, dtype=np.float32)
    N, C = logits.shape[:2]
    B = len(edges) + 1
    counts, hist = np.zeros((N, C, 4), dtype=np.int64), np.zeros((N, C, 2, B), dtype=np.int64)
    out, state = np.zeros((N, C, 5)), np.zeros((N, C), dtype=np.int64)
    for n in range(N):
        for c in range(C):
            x, t = logits[n, c].reshape(-1), target[n, c].reshape(-1)
            with np.errstate(invalid="ignore"):
                p, g = x > np.float32(0), t > np.float32(0.5)
            counts[n, c] = np.bincount(2 * (~p).astype(np.int64) + (~g).astype(np.int64), minlength=4)      # TP, FP, FN, TN
            hist[n, c] = np.bincount(g.astype(np.int64) * B + bins_of(x, edges), minlength=2 * B).reshape(2, B)
            out[n, c], state[n, c] = score_row(*counts[n, c])
    return counts, hist, out, state


def classes(logits: np.ndarray, labels: np.ndarray, first_class: int = 1, ignore_index: int = -100):
    """(counts (N, K, K) int64, out (N, P, 5) float64, state (N, P) int64) of (N, K, H, W) float32 logits against (N, H, W)
    class indices, P = K - first_class"""
    logits, labels = np.asarray(logits, dtype=np.float32), np.asarray(labels, dtype=np.int64)
    N, K = logits.shape[:2]
    P = K - first_class
    pred = np.argmax(logits, axis=1)                 # the first of equal maxima
    valid = (labels >= 0) & (labels < K) & (labels != ignore_index)
    counts = np.zeros((N, K, K), dtype=np.int64)
    out, state = np.zeros((N, P, 5)), np.zeros((N, P), dtype=np.int64)
    for n in range(N):
        v = valid[n].reshape(-1)
        counts[n] = np.bincount(labels[n].reshape(-1)[v] * K + pred[n].reshape(-1)[v], minlength=K * K).reshape(K, K)
        total = int(counts[n].sum())
        for j in range(P):
            c = first_class + j
            tp = int(counts[n, c, c])
            fp, fn = int(counts[n, :, c].sum()) - tp, int(counts[n, c, :].sum()) - tp
            out[n, j], state[n, j] = score_row(tp, fp, fn, total - tp - fp - fn)
    return counts, out, state


def curves(hist: np.ndarray, thresholds) -> dict:
    """of ONE pair's summed histograms (2, B): plain loops over the bins, float64.
    TP_j = sum of pos[b >= j], FP_j = sum of neg[b >= j], j = 0 .. B;  roc = (FPR_j, TPR_j) for j = B .. 0;
    auroc = sum_b neg[b] (sum_{b' > b} pos[b'] + pos[b] / 2) / (n_pos n_neg);  ap = sum_j (R_j - R_{j+1}) Prec_j;
    best_dice = max over j = 1 .. B - 1 of 2 TP_j / (2 TP_j + FP_j + FN_j), ties to the j nearest B / 2, then the lower j"""
    neg, pos = [int(v) for v in hist[0]], [int(v) for v in hist[1]]
    B = len(neg)
    n_pos, n_neg = sum(pos), sum(neg)
    TP = [sum(pos[j:]) for j in range(B + 1)]
    FP = [sum(neg[j:]) for j in range(B + 1)]
    nan = float("nan")
    roc = [(FP[j] / n_neg if n_neg else nan, TP[j] / n_pos if n_pos else nan) for j in range(B, -1, -1)]
    if n_pos and n_neg:
        auroc = sum(neg[b] * (TP[b + 1] + pos[b] / 2.0) for b in range(B)) / (float(n_pos) * float(n_neg))
    else:
        auroc = nan
    if n_pos:
        ap = 0.0
        for j in range(B):
            prec = TP[j] / (TP[j] + FP[j]) if TP[j] + FP[j] else 0.0
            ap += (TP[j] / n_pos - TP[j + 1] / n_pos) * prec
    else:
        ap = nan
    best, best_j = -1.0, None
    for j in range(1, B):
        den = 2 * TP[j] + FP[j] + (n_pos - TP[j])
        d = 2 * TP[j] / den if den else 0.0
        if d > best or (d == best and abs(j - B // 2) < abs(best_j - B // 2)):
            best, best_j = d, j
    th = [float(v) for v in thresholds]
    return {"roc": np.array(roc), "auroc": auroc, "ap": ap, "best_dice": best, "best_threshold": th[best_j - 1], "best_j": best_j,
            "reliability": np.array([(pos[b], pos[b] + neg[b]) for b in range(B)], dtype=np.int64)}


def ulp32(x) -> np.ndarray:
    """the spacing of float32 at |x| (of the smallest normal number below it)"""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), float(np.finfo(np.float32).tiny)).astype(np.float32)
    return np.spacing(a).astype(np.float64)
