"""Studies of the paper that are computations over a fitted model, formed on the device.

`activity_study`: the computation under the reference's user-activity figure (MFLearned.py:66-152, mf_qualitative_study; the
plotting itself is out of scope): MAP@20 of every user, averaged per bucket of how many interactions the user has.  The
reference takes the whole [users, items] score matrix to the host and loops over the users in Python; here the ranking, the
per-user values and the bucket sums come from one device call per user block (ganmf_evaluate_groups)."""
import numpy as np
import scipy.sparse as sps

from . import _lib as L


def activity_bucket_keys(bounds):
    """(keys, plotted) for ascending `bounds`: the len(bounds) + 1 labels the reference gives its users (apply_key,
    MFLearned.py:109-120) in bucket order -- '<b0', '>=b0, <b1', ..., '>=b[-2], <b[-1]', '>=b[-1]' -- and, per key, whether it is
    among the len(bounds) x-ticks of the reference's figure (build_xticks, :97-107).  The x-ticks give the last bound the label
    '>=b[-1]' INSTEAD OF '>=b[-2], <b[-1]' (and a single bound only its '<b0'), so the figure silently drops the users of that
    bucket; `plotted` is False for it."""
    b = [str(v) for v in bounds]
    if not b:
        raise ValueError("activity_bucket_keys: at least one bound")
    keys = ["<" + b[0]] + [">=" + b[i - 1] + ", <" + b[i] for i in range(1, len(b))] + [">=" + b[-1]]
    ticks = []
    for i in range(len(b)):
        if i == 0:
            ticks.append("<" + b[0])
        elif i == len(b) - 1:
            ticks.append(">=" + b[i])
        else:
            ticks.append(">=" + b[i - 1] + ", <" + b[i])
    return keys, [k in ticks for k in keys]


def activity_bucket(counts, bounds):
    """bucket index of every count: the first i with count < bounds[i], else len(bounds); a count exactly on a bound belongs to
    the bucket that starts there ('>=')"""
    return np.searchsorted(np.asarray(bounds), np.asarray(counts), side="right").astype(np.int64)


def activity_study(model, URM_test, bounds, cutoff=20, metric="MAP"):
    """Mean `metric`@`cutoff` per user-activity bucket (MFLearned.py:80-145), on the device.

    `URM_test`: users x items in evaluation orientation.  A user's activity is the row sum of URM_train + URM_test -- the sum
    of the stored VALUES, as the reference writes it, not the number of entries.  The per-user value is the reference's
    average_precision(is_relevant[:cutoff], relevant_items) (metrics.py:681-690), the device's MAP column; any other name of
    ganmf_amd._lib.EVAL_METRICS may be asked for.  Users without a test item are skipped (the reference's average_precision
    fails its own assert on 0/0 for them).

    Returns a dict: `keys` (every bucket, see activity_bucket_keys), `plotted` (whether the reference's figure shows the
    bucket), `means` (NaN for a bucket without users), `n_users` (users averaged per bucket), `bucket` (index into `keys` of
    every user), `per_user` (length n_users, NaN where skipped) and `skipped`.  Device route only: no score matrix on the
    host, and an error where the device route does not apply (a cut-off the device selection does not take)."""
    from .evaluation import EvaluatorHoldoutFast
    model._require_engine()
    col = L.EVAL_METRICS.index(metric)
    test = sps.csr_matrix(URM_test)
    train = sps.csr_matrix(model._URM_eval)
    if test.shape != train.shape:
        raise ValueError("activity_study: URM_test must be %d x %d (evaluation orientation), given %r" % (train.shape + (test.shape,)))
    keys, plotted = activity_bucket_keys(bounds)
    if len(keys) > L.EVAL_MAX_GROUPS:
        raise ValueError("activity_study: at most %d bounds" % (L.EVAL_MAX_GROUPS - 1))
    counts = np.asarray((train + test).sum(axis=1)).reshape(-1)
    bucket = activity_bucket(counts, bounds)
    ev = EvaluatorHoldoutFast(test, [cutoff], minRatingsPerUser=1)
    per_user = np.full(test.shape[0], np.nan)
    sums, sizes = np.zeros(len(keys)), np.zeros(len(keys), dtype=np.int64)
    if len(ev._users):
        got = ev._device_groups(model, keys, bucket[ev._users], True, ev._device_block())
        if got is None:
            raise RuntimeError("activity_study: cut-off %r is outside what the device route takes; there is no host route" % (cutoff,))
        sums, sizes = got[0][:, 0, col], got[1]
        per_user[ev._users] = got[2][:, 0, col]
    with np.errstate(invalid="ignore", divide="ignore"):
        means = np.where(sizes > 0, sums / np.maximum(sizes, 1), np.nan)
    return dict(keys=keys, plotted=plotted, means=means, n_users=sizes, bucket=bucket, per_user=per_user,
                skipped=int(test.shape[0] - len(ev._users)), cutoff=cutoff, metric=metric)


def discriminator_summary(real, generated, m=None, logits=False):
    """The host arithmetic of discriminator_study on two per-row vectors (float64).
    logits=False (GANMF, energies): energy_real / energy_generated, their means, and with the hinge multiplier `m` the term the
    discriminator loss adds to the real rows' error, hinge = m * mean_real - mean_generated (GANMF.py:69-70, F12 of SURVEY.md), and
    hinge_active = hinge > 0; both None when `m` is None.
    logits=True (DisGANMF): p_real / p_generated = sigmoid(logit), their means, and accuracy = (share of real logits > 0 + share
    of generated logits < 0) / 2."""
    real = np.asarray(real, dtype=np.float64).reshape(-1)
    generated = np.asarray(generated, dtype=np.float64).reshape(-1)
    mean = lambda v: float(v.mean()) if v.size else float("nan")
    if logits:
        p_real, p_gen = 1.0 / (1.0 + np.exp(-real)), 1.0 / (1.0 + np.exp(-generated))
        acc = 0.5 * (mean((real > 0).astype(np.float64)) + mean((generated < 0).astype(np.float64)))
        return dict(p_real=p_real, p_generated=p_gen, mean_p_real=mean(p_real), mean_p_generated=mean(p_gen), accuracy=acc)
    out = dict(energy_real=real, energy_generated=generated, mean_real=mean(real), mean_generated=mean(generated),
               hinge=None, hinge_active=None)
    if m is not None:
        out["hinge"] = float(m) * out["mean_real"] - out["mean_generated"]
        out["hinge_active"] = bool(out["hinge"] > 0)
    return out


def discriminator_study(model, row_ids=None):
    """Real against generated rows as the fitted discriminator sees them, for the generator rows `row_ids` (training orientation;
    None: all).  The per-row vectors come from the device (ganmf_discriminate); this function only averages them, see
    discriminator_summary.  GANMF: the EBGAN energies and the hinge m * mean_real - mean_generated, with m from model.config (a
    model restored by loadModel has no config: hinge and hinge_active are None).  DisGANMF: sigmoid(logit) and the accuracy."""
    model._require_engine()
    if hasattr(model, "discriminator_logits"):
        return discriminator_summary(model.discriminator_logits(row_ids), model.discriminator_logits(row_ids, generated=True),
                                     logits=True)
    m = model.config.get("m") if isinstance(getattr(model, "config", None), dict) else None
    return discriminator_summary(model.discriminator_energy(row_ids), model.discriminator_energy(row_ids, generated=True), m=m)
