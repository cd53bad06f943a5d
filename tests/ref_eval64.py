"""Host restatements of the validation-pass kernels (csrc/eval.hip): Caffe's Accuracy layer over the channel axis with integer
counts, and Solver::Test's float32 running sum of an output blob.  No GPU, no package import: numpy only."""
import numpy as np


def accuracy_counts(scores, labels, top_k=1, ignore_label=None):
    """scores (N, C, H, W), labels (N, 1, H, W) or (N, H, W) class ids -> (correct, valid, correct_c (C,), n_c (C,)), integers.
    BVLC master's rule: a labelled pixel is correct iff fewer than top_k channels j != label score >= the label's (ties count
    against the label); a pixel whose label equals ignore_label is skipped; a label outside [0, C) is valid and wrong."""
    x = np.asarray(scores, np.float32)
    n, c, h, w = x.shape
    lab = np.asarray(labels).reshape(n, h, w).astype(np.int64)
    correct = valid = 0
    correct_c, n_c = np.zeros(c, np.int64), np.zeros(c, np.int64)
    for i in range(n):
        for y in range(h):
            for xx in range(w):
                l = int(lab[i, y, xx])
                if ignore_label is not None and l == int(ignore_label):
                    continue
                valid += 1
                if not 0 <= l < c:
                    continue
                v = x[i, :, y, xx]
                ge = int(np.sum(v >= v[l])) - 1      # (v[l] >= v[l] itself)
                n_c[l] += 1
                if ge < top_k:
                    correct += 1
                    correct_c[l] += 1
    return correct, valid, correct_c, n_c


def accuracy(scores, labels, top_k=1, ignore_label=None):
    """-> (float32 accuracy, float32 per-class accuracies (C,)) as the layer's two tops: 0 where nothing was counted."""
    ok, valid, ok_c, n_c = accuracy_counts(scores, labels, top_k, ignore_label)
    acc = np.float32(ok) / np.float32(valid) if valid else np.float32(0)
    per = np.zeros(len(n_c), np.float32)
    nz = n_c > 0
    per[nz] = ok_c[nz].astype(np.float32) / n_c[nz].astype(np.float32)
    return np.float32(acc), per


def running_sum(blobs):
    """float32 sum of a sequence of equally shaped arrays in call order, one add per element per term: test_score[] += result."""
    acc = np.zeros(np.asarray(blobs[0]).shape, np.float32)
    for b in blobs:
        acc = (acc + np.asarray(b, np.float32)).astype(np.float32)
    return acc


def test_mean(blobs):
    """Solver::Test's mean_score: the running sum divided by the number of forwards, in float32."""
    return (running_sum(blobs) / np.float32(len(blobs))).astype(np.float32)


test_mean.__test__ = False
