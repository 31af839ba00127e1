"""CAAE recommender -- host mirror of the reference class (GANRec/CAAE.py:22-399): a pairwise discriminator over (user, positive,
negative) triples and two sigmoid MLP generators G and G' over the user's profile, all trained by plain SGD; G's negatives and G''s
negatives feed the discriminator, the discriminator's rewards feed both generators' policy gradients.  Same constructor, fit()
keyword arguments, return value, scoring and early-stopping hooks as the reference, so it can stand in for `GANRec.CAAE.CAAE`.  Every
number is produced by libganmf_hip.so (ganmf_caae_* on a GANMF_MODEL_CAAE handle); this file holds the epoch loop, the host
replay of the reference's draws and bookkeeping."""
import os
import time
from datetime import datetime

import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .base import BaseRecommender
from .CFGAN import non_interactions, pack_mask_rows
from .device_scoring import DeviceScoringMixin
from .early_stopping import EarlyStoppingScheduler
from .GANMF import _SessionShim, _TensorRef, glorot_uniform

SAMPLERS = ("device", "numpy")


def nu_size(n_free, S):
    """Size of the subset Nu of n_free non-interactions (CAAE.py:280): S enters as a Python double."""
    return int(n_free * S)


def policy_draws(urm):
    """n_s = 2 * median profile length, the median cast to int32 first (CAAE.py:197,293)"""
    return 2 * int(np.median(np.ediff1d(sps.csr_matrix(urm).indptr)).astype(np.int32))


def init_weights(seed, num_users, num_items, num_factors, g_layers, g_units):
    """Host initialisation from RandomState(seed) in TF variable order -- D (disc_user_embeddings, disc_item_embeddings, disc_item_bias),
    then G, then G' (per layer kernel then bias): embeddings and kernels Glorot-uniform, disc_item_bias uniform +-sqrt(3 / I) (TF's
    default initialiser of a 1-D variable: glorot_uniform with fan_in = fan_out = I), dense biases zero (they draw nothing).  G' is
    built with G's depth and width (CAAE.py:137).  Returns {'D': [...], 'G': [...], 'G_prime': [...]} in tensor-id order."""
    rng = np.random.RandomState(seed)
    out = {'D': [glorot_uniform(rng, (num_users, num_factors)), glorot_uniform(rng, (num_items, num_factors))]}
    lim = np.sqrt(3.0 / num_items)
    out['D'].append(rng.uniform(-lim, lim, size=num_items).astype(np.float32))
    for key in ('G', 'G_prime'):
        out[key] = []
        fan = num_items
        for _ in range(g_layers):
            out[key] += [glorot_uniform(rng, (fan, g_units)), np.zeros(g_units, dtype=np.float32)]
            fan = g_units
        out[key] += [glorot_uniform(rng, (fan, num_items)), np.zeros(num_items, dtype=np.float32)]
    return out


def search_cdf(cdf_rows, rows, samples):
    """cython_utils.pyx:166-181 per sample: the first index of cdf_rows[rows[i]] whose value is >= samples[i], clamped to I - 1"""
    out = np.zeros(len(rows), dtype=np.int32)
    last = cdf_rows.shape[1] - 1
    for i, (r, a) in enumerate(zip(rows, samples)):
        out[i] = min(int(np.searchsorted(cdf_rows[r], a, side='left')), last)
    return out


def random_choice_numpy(cdf, cdf2=None, size=1, custom_ordered_rows=None):
    """cython_utils.pyx:74-104 replayed from numpy's global stream: one np.random.random(...).astype(float32) call for every row (twice
    as many with cdf2: the first half searches cdf, the second cdf2)"""
    rows = np.repeat(np.arange(cdf.shape[0]), size) if custom_ordered_rows is None else np.asarray(custom_ordered_rows)
    n = len(rows)
    samples = np.random.random(n if cdf2 is None else 2 * n).astype(np.float32)
    first = search_cdf(cdf, rows, samples[:n])
    if cdf2 is None:
        return first
    return first, search_cdf(cdf2, rows, samples[n:])


def run_epoch_numpy(backend, order, users_of, items_of, free, num_users, num_items, d_steps, g_steps, gpr_steps, d_bsize, m_batch,
                    n_s, S):
    """One epoch with the reference's own draws (CAAE.py:220-337), taken from numpy's global stream in its order: the in-place shuffle
    of `order` (CSR positions; the list stays shuffled from epoch to epoch, as all_interactions does), per discriminator pass one
    random(2 nnz), per generator step choice(users, replace=False), one weighted choice per user and random(m n_s), per step of G'
    choice(users) and random(m n_s).  `backend` does the arithmetic: cdf_all(which) -> [U, I], cdf_rows(which, users) -> [m, I],
    d_step(u, i, j) -> loss, g_step(which, users, nu_bool_or_None, items) -> loss.  Returns the three loss lists."""
    np.random.shuffle(order)
    users, pos = users_of[order], items_of[order]
    cdf_g, cdf_gpr = backend.cdf_all(0), backend.cdf_all(1)
    prob_gpr = np.diff(cdf_gpr.astype(np.float64), axis=1, prepend=0.0)
    all_users = np.arange(num_users, dtype=np.int32)
    dl, gl, pl = [], [], []
    for _ in range(d_steps):
        g_neg, gpr_neg = random_choice_numpy(cdf_g, cdf_gpr, custom_ordered_rows=users)
        for s in range(0, len(order), d_bsize):
            e = min(s + d_bsize, len(order))
            dl.append(backend.d_step(users[s:e], pos[s:e], g_neg[s:e]))
            dl.append(backend.d_step(users[s:e], pos[s:e], gpr_neg[s:e]))
    for _ in range(g_steps):
        uids = np.random.choice(all_users, size=m_batch, replace=False)
        nu = np.zeros((m_batch, num_items), dtype=bool)
        for i, u in enumerate(uids):
            k = nu_size(len(free[u]), S)
            if k:
                p = prob_gpr[u, free[u]]
                nu[i, np.random.choice(free[u], size=k, p=p / p.sum(), replace=False)] = True
        items = random_choice_numpy(backend.cdf_rows(0, uids), size=n_s).reshape(m_batch, -1)
        gl.append(backend.g_step(0, uids, nu, items))
    for _ in range(gpr_steps):
        uids = np.random.choice(all_users, size=m_batch)
        items = random_choice_numpy(backend.cdf_rows(1, uids), size=n_s).reshape(m_batch, -1)
        pl.append(backend.g_step(1, uids, None, items))
    return dl, gl, pl


class _EngineBackend(object):
    def __init__(self, engine):
        self.engine = engine

    def cdf_all(self, which):
        return self.engine.caae_cdf(which)[0]

    def cdf_rows(self, which, users):
        return self.engine.caae_cdf(which, users)[0]

    def d_step(self, u, i, j):
        return self.engine.caae_d_step(u, i, j)

    def g_step(self, which, users, nu, items):
        return self.engine.caae_g_step(which, users, pack_mask_rows(nu) if nu is not None else None, items)


class CAAE(DeviceScoringMixin, BaseRecommender):
    """Reference quirks kept:
      * `mode` is stored (as `given_mode`) and ignored: the matrix is never transposed;
      * gpr_layers and gpr_units are accepted, stored in `config` and never read: G' is built with g_layers / g_units (CAAE.py:137);
      * the auto-encoder mask carries the stored profile values (not ones) plus 1 on Nu;
      * S enters as a Python double: the size of Nu is int(n_free * S) (`nu_size`);
      * n_s = 2 * median profile length; m_batch distinct users for G, with replacement for G';
      * fit() returns epoch - 1 when early stopping fired, else epochs + 1;
      * saveModel(folder_path, file_name) writes the Saver bundle only, holding the D, the G and the G' variables:
        D/disc_user_embeddings, D/disc_item_embeddings, D/disc_item_bias, G/g_layer_%d/{kernel,bias}, G/g_reconstruction/{kernel,bias},
        G_prime/gpr_layer_%d/{kernel,bias}, G_prime/gpr_reconstruction/{kernel,bias}.
    Departures:
      * _compute_item_score scores the users it is asked for; the reference scores rows [0, len) whatever ids it gets (CAAE.py:391-392);
      * log sigmoid is computed as min(y, 0) - log1p(exp(-|y|)), which does not overflow where log(sigmoid(y)) does;
      * sampler="device" (default) draws everything on the device from a counter-based generator keyed by (seed, epoch, stream, pass /
        step, index): the reference's distributions (Nu by Efraimidis-Spirakis keys, i.e. successive sampling), but not numpy's stream;
        Nu is weighted by G' at the parameters it has when the generator step runs, which inside an epoch are its epoch-start ones.
        sampler="numpy" replays the reference's draws from numpy's global stream on the host (`run_epoch_numpy`) and runs the epoch step
        by step on explicit indices; Nu's weights are then the differences of the downloaded epoch-start CDF;
      * weights are initialised on the host from RandomState(seed) (`init_weights`), not from TF's graph seed;
      * stored zeros of URM_train are dropped, so "non-interaction" means the same on the host and on the device;
      * num_factors is at most 256, d_bsize at most 16384, m_batch at most the number of users, and the median profile must not be
        empty (n_s >= 1)."""
    RECOMMENDER_NAME = 'CAAE'
    SCORE_CONTRACTS = ("ganmf",)

    def __init__(self, URM_train, verbose=False, mode='user', seed=1234, is_experiment=False, device=0, sampler="device"):
        if sampler not in SAMPLERS:
            raise ValueError("sampler must be one of %r, given %r" % (SAMPLERS, sampler))
        URM_train = sps.csr_matrix(URM_train, dtype=np.float32)
        URM_train.sum_duplicates()
        URM_train.eliminate_zeros()
        URM_train.sort_indices()
        self.given_mode = mode
        self.mode = 'user'          # what the device scoring surface reads: users are rows, always
        self.URM_train = self._URM_eval = self._URM_fit = URM_train
        self.num_users, self.num_items = URM_train.shape
        self.n_users, self.n_items = URM_train.shape
        self.config = None
        self.seed = seed
        self.verbose = verbose
        self.device = device
        self.sampler = sampler
        self.score_contract = "ganmf"
        self.logsdir = os.path.join('plots', self.RECOMMENDER_NAME, datetime.now().strftime("%Y%m%d-%H%M%S"))
        self.is_experiment = is_experiment
        if not self.is_experiment:
            os.makedirs(self.logsdir, exist_ok=True)
        self.items_to_ignore_flag = False
        self.items_to_ignore_ID = np.array([], dtype=int)
        self.filterTopPop = False
        self.filterTopPop_ItemsID = np.array([], dtype=int)
        self.initial_weights = None     # optional {'D': [...], 'G': [...], 'G_prime': [...]} in tensor-id order (init_weights' layout)
        self.engine = None
        self.params = None
        self.sess = None
        self._stop_training = False
        self.train_d_loss, self.train_pg_loss, self.train_ng_loss = [], [], []

    # ---- engine plumbing -----------------------------------------------------------------------
    def _names(self):
        d = ['D/disc_user_embeddings', 'D/disc_item_embeddings', 'D/disc_item_bias']
        g, gp = [], []
        for l in range(self.g_layers):
            g += ['G/g_layer_%d/kernel' % l, 'G/g_layer_%d/bias' % l]
            gp += ['G_prime/gpr_layer_%d/kernel' % l, 'G_prime/gpr_layer_%d/bias' % l]
        g += ['G/g_reconstruction/kernel', 'G/g_reconstruction/bias']
        gp += ['G_prime/gpr_reconstruction/kernel', 'G_prime/gpr_reconstruction/bias']
        return d, g, gp

    def _get(self, tid):
        a = self.engine.get_tensor(tid)
        one_d = tid == L.T_CAAE_ITEM_BIAS or (tid >= L.T_CAAE_G0 and tid % 2 == 1)      # biases are 1-D in the reference
        return a.reshape(-1) if one_d else a

    def _build(self, num_factors, g_layers, g_units, d_bsize=1024, m_batch=32, lmbda=0.5, beta=1e-4, lr=1e-4, S=0.3):
        from .engine import Engine
        if g_layers < 1 or g_units < 1:
            raise ValueError("CAAE needs g_layers >= 1 and g_units >= 1")
        if not 1 <= num_factors <= L.CAAE_MAX_FACTORS:
            raise ValueError("CAAE needs 1 <= num_factors <= %d" % L.CAAE_MAX_FACTORS)
        if not 1 <= d_bsize <= L.CAAE_MAX_D_BSIZE:
            raise ValueError("CAAE needs 1 <= d_bsize <= %d" % L.CAAE_MAX_D_BSIZE)
        if not 1 <= m_batch <= self.num_users:
            raise ValueError("CAAE draws m_batch distinct users: 1 <= m_batch <= %d" % self.num_users)
        n_s = policy_draws(self._URM_fit)
        if n_s < 1:
            raise ValueError("CAAE draws 2 * median profile length items per user: the median profile is empty")
        self.num_factors, self.g_layers, self.g_units, self.d_bsize, self.m_batch, self.n_s, self.S = (
            num_factors, g_layers, g_units, d_bsize, m_batch, n_s, S)
        if self.engine is not None:
            self.engine.close()
        self.engine = Engine(self.num_users, self.num_items, num_factors, 1, 1, model=L.MODEL_CAAE, device=self.device)
        self.engine.set_urm(self._URM_fit)
        self.engine.set_seen(self._URM_eval)
        lens = np.diff(self._URM_fit.indptr)
        k_rows = [nu_size(self.num_items - int(n), S) for n in lens]
        self.engine.caae_init(g_units, g_layers, d_bsize, m_batch, n_s, lmbda, beta, lr, self.seed, k_rows)
        self._reset_score_filter()
        d, g, gp = self._names()
        self.params = {'D': [_TensorRef(t, n) for t, n in zip((L.T_USER_EMB, L.T_ITEM_EMB, L.T_CAAE_ITEM_BIAS), d)],
                       'G': [_TensorRef(L.T_CAAE_G0 + i, n) for i, n in enumerate(g)],
                       'G_prime': [_TensorRef(L.T_CAAE_GPR0 + i, n) for i, n in enumerate(gp)]}
        self.sess = _SessionShim(self)

    def _all_refs(self):
        return self.params['D'] + self.params['G'] + self.params['G_prime']

    def _init_weights(self):
        w = self.initial_weights
        if w is None:
            w = init_weights(self.seed, self.num_users, self.num_items, self.num_factors, self.g_layers, self.g_units)
        for key in ('D', 'G', 'G_prime'):
            for ref, a in zip(self.params[key], w[key]):
                self.engine.set_tensor(ref.tid, np.asarray(a, dtype=np.float32))

    # ---- fit (CAAE.py:123-369) --------------------------------------------------------------------
    def fit(self, epochs=300, d_steps=1, g_steps=1, gpr_steps=1, g_layers=1, g_units=20, gpr_layers=1, gpr_units=20,
            num_factors=10, d_bsize=1024, m_batch=32, lmbda=0.5, beta=1e-4, lr=1e-4, S=0.3, allow_worse=None, freq=None,
            after=0, metrics=['MAP'], sample_every=None, validation_evaluator=None, validation_set=None):
        self.config = dict(locals())
        del self.config['self']
        self._build(num_factors, g_layers, g_units, d_bsize=d_bsize, m_batch=m_batch, lmbda=lmbda, beta=beta, lr=lr, S=S)
        self._init_weights()

        self._stop_training = False
        watcher = None
        if allow_worse is not None and validation_evaluator is not None:
            watcher = EarlyStoppingScheduler(self, evaluator=validation_evaluator, allow_worse=allow_worse, freq=freq,
                                             metrics=metrics, after=after)
        self.train_d_loss, self.train_pg_loss, self.train_ng_loss = [], [], []
        if self.verbose:
            print('Starting training...')
        fit_t0 = window_t0 = time.time()
        epoch = 1
        if self.sampler == "numpy":
            urm = self._URM_fit
            order = np.arange(urm.nnz)
            users_of = np.repeat(np.arange(self.num_users, dtype=np.int32), np.diff(urm.indptr))
            free = non_interactions(urm)
            backend = _EngineBackend(self.engine)
        while not self._stop_training and epoch < epochs + 1:
            if self.sampler == "numpy":
                losses = run_epoch_numpy(backend, order, users_of, urm.indices, free, self.num_users, self.num_items, d_steps, g_steps,
                                         gpr_steps, d_bsize, m_batch, self.n_s, S)
            else:
                losses = self.engine.caae_epoch(epoch, d_steps, g_steps, gpr_steps)
            for store, l in zip((self.train_d_loss, self.train_pg_loss, self.train_ng_loss), losses):
                store.append(np.mean(l) if len(l) else np.nan)
            if validation_set is not None and sample_every is not None and epoch % sample_every == 0:
                elapsed = time.time() - window_t0
                print('Epoch : {:d}. Total: {:.2f} secs, {:.2f} secs/epoch.'.format(epoch, elapsed, elapsed / sample_every))
                print(validation_evaluator.evaluateRecommender(self)[1])
                window_t0 = time.time()
            if watcher is not None:
                watcher(epoch)
                if self._stop_training:
                    print('Training stopped, epoch:', epoch)
            epoch += 1
        if self.verbose:
            print('Training took {:.2f} seconds'.format(time.time() - fit_t0))
        return epoch - 1 if self._stop_training else epoch

    # ---- hooks used by EarlyStoppingScheduler (CAAE.py:371-380) ---------------------------------
    def stop_fit(self):
        self._stop_training = True

    def save_current_model(self):
        self.engine.snapshot_best()

    def load_model(self):
        self.engine.restore_best()

    def _require_engine(self):
        if self.engine is None:
            raise RuntimeError("CAAE: model has no device state; call fit() or load_bundle() first")

    # ---- persistence (CAAE.py:397-399) ------------------------------------------------------------
    def saveModel(self, folder_path, file_name):
        from .tf_bundle import write_bundle
        self._require_engine()
        os.makedirs(folder_path, exist_ok=True)
        write_bundle(os.path.join(folder_path, file_name), {ref.name: self.sess.run(ref) for ref in self._all_refs()})

    def load_bundle(self, folder_path, file_name):
        """Inverse of saveModel: the factors, the depth and the width are read from the bundle's shapes."""
        from .tf_bundle import read_bundle
        data = read_bundle(os.path.join(folder_path, file_name))
        g_layers = len([k for k in data if k.startswith('G/g_layer_') and k.endswith('/kernel')])
        g_units = data['G/g_reconstruction/kernel'].shape[0]
        self._build(data['D/disc_user_embeddings'].shape[1], g_layers, g_units, m_batch=min(32, self.num_users))
        for ref in self._all_refs():
            if ref.name not in data:
                raise KeyError("%s: checkpoint has no tensor %r" % (self.RECOMMENDER_NAME, ref.name))
            self.engine.set_tensor(ref.tid, data[ref.name])
