"""``metrics.EpochMetrics`` (``csrc/k_metrics.hip``) on the device.

* every case of ``tests/golden/epoch_metrics.json`` (the reference's ``EnsembleTrainer.validate`` on canned logits),
  fed in the recorded batch splits from ``capacity=8`` so the buffers grow on the way: ``compute()`` equals the
  recorded dict -- integers, thresholds, confusion matrix and absent keys exactly, floats within 1e-12, the loss
  exactly (one fp64 add per step, in stream order) -- and the stored probabilities match torch's CPU softmax at the
  project's fp32 tolerance (rtol 1e-3, atol 1e-5).  The golden's inputs keep the metrics independent of a
  probability's last bit (asserted by its generator).
* self-consistency past those separation rules: 4099 random rows with ``|z1 - z0|`` up to 40 (probabilities that
  saturate to 1.0 or fall to 1e-17, exact and argmax ties, unlabelled rows): the device's counts and U2 equal
  numpy's from the device's OWN stored probabilities and tags exactly, and two ``compute()`` calls return the
  same bits.
* ``reset()`` and a shorter epoch: the rows of the longer one past N are not read.
"""
import numpy as np
import pytest
import torch

import epoch_metrics_helpers as eh
from deepfake_amd.metrics import TAG_LABEL, TAG_PRED, TAG_VALID, EpochMetrics

pytestmark = pytest.mark.gpu


def _feed(em, name, dev, with_loss=True):
    A, _ = eh.load()
    z, y, losses = A[f"{name}/logits"], A[f"{name}/labels"], A[f"{name}/losses"]
    o, fed = 0, []
    for i, b in enumerate(A[f"{name}/batches"].tolist()):
        loss = torch.tensor(losses[i], dtype=torch.float32, device=dev) if with_loss else None
        assert float(np.float32(losses[i])) == float(losses[i])  # the recorded losses are fp32 values
        em.update(torch.from_numpy(z[o:o + b]).to(dev), torch.from_numpy(y[o:o + b]).to(dev), loss)
        fed.append((float(losses[i]), b))
        o += b
    assert o == len(z)
    return fed


@pytest.mark.parametrize("name", eh.case_names())
def test_epoch_metrics_match_reference(cuda, name):
    A, R = eh.load()
    ref = R["cases"][name]
    em = EpochMetrics(cuda, capacity=8)
    fed = _feed(em, name, cuda)
    n = len(A[f"{name}/labels"])
    assert em.n == n and em.capacity >= n and (n <= 8 or em.capacity > 8)
    got = em.compute()
    print(name, got)
    eh.assert_metrics(got, ref["validate"], what=name)
    if "train_epoch" in ref:
        eh.assert_metrics(got, ref["train_epoch"], keys=list(ref["train_epoch"]), what=name)
    eh.assert_metrics(em.compute(average="weighted"), ref["weighted"], keys=list(ref["weighted"]), what=name)
    tot = cnt = 0.0
    for loss, b in fed:  # src/train.py:128,133
        tot += loss * b
        cnt += b
    assert em.compute(loss_mean="per_sample")["loss"] == tot / cnt
    torch.testing.assert_close(em.probs().cpu(), torch.from_numpy(A[f"{name}/probs"]), rtol=1e-3, atol=1e-5)
    assert torch.equal(em.labels().cpu(), torch.from_numpy(A[f"{name}/labels"]))
    z = A[f"{name}/logits"]
    assert torch.equal(em.preds().cpu(), torch.from_numpy((z[:, 1] > z[:, 0]).astype(np.int64)))


def test_counts_consistent_with_stored_rows(cuda):
    g = torch.Generator().manual_seed(4099)
    n = 4099
    z = torch.randn(n, 2, generator=g) * 3
    z[:, 1] = z[:, 0] + (torch.rand(n, generator=g) * 80 - 40)
    z[::7] = z[3]  # exact ties
    z[5::11, 1] = z[5::11, 0]  # argmax ties
    y = torch.randint(0, 2, (n,), generator=g)
    y[2::13] = -1
    em = EpochMetrics(cuda, capacity=8)
    for o in range(0, n, 1000):
        em.update(z[o:o + 1000].to(cuda), y[o:o + 1000].to(cuda))
    c1 = em.counts()
    m1, m2 = em.compute(), em.compute()
    assert m1 == m2 and c1 == em.counts()
    probs, tags = em.probs().cpu().numpy(), em.tags().cpu().numpy().astype(np.int64)
    # 1 / (1 + e^-40) rounds to 1.0; e^-40 itself is an fp32 number (4.2e-18), so the low side does not reach 0.0
    assert probs.max() == 1.0 and 0.0 < probs.min() < 1e-15 and (probs == 1.0).sum() > 100
    labels = np.where(tags & TAG_VALID, tags & TAG_LABEL, -1)
    assert np.array_equal(labels, y.numpy())
    preds = (tags & TAG_PRED) >> 1
    assert np.array_equal(preds, (z[:, 1] > z[:, 0]).numpy().astype(np.int64))
    want = eh.numpy_counts(probs, labels, preds)
    for k, v in want.items():
        assert c1[k] == v, (k, c1[k], v)
    assert c1["loss_sum"] == 0.0 and m1["loss"] == 0.0  # no loss was given
    # a caller's own thresholds, 32 of them
    thr = np.linspace(0.0, 1.0, 32, dtype=np.float32)
    c3 = em.counts(thr)
    want = eh.numpy_counts(probs, labels, preds, thr)
    assert c3["tp_t"] == want["tp_t"] and c3["fp_t"] == want["fp_t"] and c3["u2"] == want["u2"]
    with pytest.raises(ValueError):
        em.counts(np.linspace(0.0, 1.0, 33))


def test_reset_then_shorter_epoch(cuda):
    _, R = eh.load()
    em = EpochMetrics(cuda, capacity=8)
    _feed(em, "n1031", cuda)
    cap = em.capacity
    em.reset()
    assert em.n == 0 and em.compute()["confusion_matrix"] == []  # N == 0: all-zero counts
    _feed(em, "n63", cuda)
    assert em.capacity == cap
    eh.assert_metrics(em.compute(), R["cases"]["n63"]["validate"], what="n63 after n1031")


def test_update_rejects_other_shapes(cuda):
    em = EpochMetrics(cuda)
    with pytest.raises(ValueError):
        em.update(torch.zeros(4, 3, device=cuda), torch.zeros(4, dtype=torch.long, device=cuda))
    with pytest.raises(ValueError):
        em.compute(loss_mean="median")
    assert em.n == 0
