"""CFGAN recommender -- host mirror of the reference class (GANRec/CFGAN.py:22-372): an MLP generator over the row's own profile, an
MLP discriminator over [profile | profile-shaped input], sigmoid cross-entropy, TF-1 Adam, and per-epoch zero-reconstruction /
partial-masking masks.  Same constructor, fit() keyword arguments, return value, scoring and early-stopping hooks as the reference,
so it can stand in for `GANRec.CFGAN.CFGAN`.  Every number is produced by libganmf_hip.so (ganmf_cfgan_* on a GANMF_MODEL_CFGAN
handle); this file holds the epoch loop, the host mask sampler and bookkeeping."""
import os
import time
from datetime import datetime

import numpy as np
import scipy.sparse as sps

from . import _lib as L
from .base import BaseRecommender
from .device_scoring import DeviceScoringMixin
from .early_stopping import EarlyStoppingScheduler
from .GANMF import _SessionShim, _TensorRef

SCHEMES = ("ZR", "PM", "ZP")
MASK_SAMPLERS = ("device", "numpy")


def mask_size(n, ratio):
    """Subset size the reference draws from n non-interactions: its Cython compute_masks takes the ratio as a C `float`, so the
    product is formed with the float32-rounded ratio (0.7 of 10 gives 6, not 7)."""
    return int(n * float(np.float32(ratio)))


def non_interactions(urm):
    """per row, the ascending columns without a stored non-zero (what the reference's get_non_interactions returns)"""
    urm = sps.csr_matrix(urm)
    out = []
    for u in range(urm.shape[0]):
        row = np.zeros(urm.shape[1], dtype=bool)
        cols = urm.indices[urm.indptr[u]:urm.indptr[u + 1]]
        row[cols[urm.data[urm.indptr[u]:urm.indptr[u + 1]] != 0]] = True
        out.append(np.nonzero(~row)[0])
    return out


def pack_mask_rows(dense):
    """bool / 0-1 [rows, I] -> uint32 [rows, ceil(I / 32)]: bit (j & 31) of word (j >> 5) is column j, tail bits 0
    (np.packbits(..., bitorder='little') viewed as little-endian 32-bit words)"""
    dense = np.asarray(dense).astype(bool)
    rows, n = dense.shape
    words = (n + 31) // 32
    padded = np.zeros((rows, words * 32), dtype=bool)
    padded[:, :n] = dense
    return np.packbits(padded, axis=1, bitorder='little').reshape(rows, words, 4).copy().view('<u4').reshape(rows, words).astype(np.uint32)


def unpack_mask_rows(words, n):
    """inverse of pack_mask_rows: uint32 [rows, ceil(n / 32)] -> bool [rows, n]"""
    w = np.ascontiguousarray(words, dtype='<u4')
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder='little')
    return bits[:, :n].astype(bool)


def draw_masks_numpy(urm, scheme, zr_ratio, rng=None, free=None):
    """The reference's compute_masks replayed on the host from numpy's global stream (or `rng`): per row in order, the ZR draw
    (schemes ZR, ZP) then the PM draw (schemes PM, ZP), each np.random.choice(non-interactions, size, replace=False) with BOTH
    sizes formed from zr_ratio (the reference never reads zp_ratio).  `free`: non_interactions(urm) when the caller holds it (the
    reference forms it once per fit).  Returns (zr, pm) bool [rows, I]; an unused plane is all False."""
    if scheme not in SCHEMES:
        raise ValueError("scheme must be one of %r, given %r" % (SCHEMES, scheme))
    rng = np.random if rng is None else rng
    urm = sps.csr_matrix(urm)
    zr = np.zeros(urm.shape, dtype=bool)
    pm = np.zeros(urm.shape, dtype=bool)
    for u, cols in enumerate(non_interactions(urm) if free is None else free):
        k = mask_size(len(cols), zr_ratio)
        if scheme in ("ZP", "ZR"):
            zr[u, rng.choice(cols, size=k, replace=False)] = True
        if scheme in ("ZP", "PM"):
            pm[u, rng.choice(cols, size=k, replace=False)] = True
    return zr, pm


def init_weights(seed, num_items, d_nodes, d_layers, g_nodes, g_layers):
    """Host initialisation from RandomState(seed) in TF variable order -- the discriminator's layers then the generator's, kernel then
    bias each: kernels uniform +-sqrt(6 / (fan_in + fan_out)), biases uniform +-0.01 (CFGAN.py:50,59-60).  Returns
    {'D': [arrays], 'G': [arrays]} in tensor-id order."""
    rng = np.random.RandomState(seed)

    def layer(fan_in, fan_out):
        s = np.sqrt(6.0 / (fan_in + fan_out))
        return [rng.uniform(-s, s, size=(fan_in, fan_out)).astype(np.float32),
                rng.uniform(-0.01, 0.01, size=fan_out).astype(np.float32)]
    out = {'D': [], 'G': []}
    fan = 2 * num_items
    for _ in range(d_layers):
        out['D'] += layer(fan, d_nodes)
        fan = d_nodes
    out['D'] += layer(fan, 1)
    fan = num_items
    for _ in range(g_layers):
        out['G'] += layer(fan, g_nodes)
        fan = g_nodes
    out['G'] += layer(fan, num_items)
    return out


class CFGAN(DeviceScoringMixin, BaseRecommender):
    """Reference quirks kept:
      * compute_masks sizes BOTH draws by zr_ratio; zp_ratio is accepted, stored in `config` and never read;
      * the ratio passes through a C float: the size is int(n * float(np.float32(zr_ratio))) (`mask_size`), formed on the host;
      * fit() returns epoch - 1 when early stopping fired, else epochs + 1;
      * saveModel(folder_path, file_name) writes the Saver bundle only (no build_params.pkl), holding the D then the G variables:
        discriminator/D_hidden_%d/{kernel,bias}, discriminator/D_output/{kernel,bias}, generator/G_hidden_%d/{kernel,bias},
        generator/G_output/{kernel,bias}.
    Departures:
      * 'LeakyReLU' raises ValueError (it is in no search space and not among the library's activations);
      * d_layers and g_layers must be >= 1;
      * world_size > 1 and the bf16 / fp16 MFMA flags are refused (single GPU, fp32-accurate products);
      * mask_sampler="device" (default) draws the masks on the device from a counter-based generator keyed by (seed, epoch, plane,
        row, column): uniform subsets of the reference's sizes, but not numpy's stream.  mask_sampler="numpy" replays compute_masks
        from numpy's global stream on the host (`draw_masks_numpy`) and uploads the planes every epoch;
      * weights are initialised on the host from RandomState(seed) (`init_weights`), not from TF's graph seed;
      * stored zeros of URM_train are dropped, so "non-interaction" means the same on the host and on the device."""
    RECOMMENDER_NAME = 'CFGAN'
    SCORE_CONTRACTS = ("ganmf",)

    def __init__(self, URM_train, mode='user', seed=1234, verbose=False, is_experiment=False, device=0, mask_sampler="device",
                 world_size=None, mfma=None):
        if mode not in ['user', 'item']:
            raise ValueError('Accepted training modes are `user` and `item`. Given was {}.', mode)
        if mask_sampler not in MASK_SAMPLERS:
            raise ValueError("mask_sampler must be one of %r, given %r" % (MASK_SAMPLERS, mask_sampler))
        if world_size is not None and world_size > 1:
            raise ValueError("CFGAN trains on one GPU: world_size %r is refused" % (world_size,))
        if mfma in ("bf16", "f16"):
            raise ValueError("CFGAN runs the fp32-accurate products only: mfma=%r is refused" % (mfma,))
        self.mode = mode
        URM_train = sps.csr_matrix(URM_train, dtype=np.float32)
        URM_train.sum_duplicates()
        URM_train.eliminate_zeros()
        self._URM_eval = URM_train
        self._URM_fit = URM_train.T.tocsr() if mode == 'item' else URM_train
        self._URM_fit.sort_indices()
        self.URM_train = self._URM_fit
        self.num_users, self.num_items = self.URM_train.shape
        self.n_users, self.n_items = URM_train.shape
        self.config = None
        self.seed = seed
        self.verbose = verbose
        self.device = device
        self.mask_sampler = mask_sampler
        self.mfma = mfma
        self.score_contract = "ganmf"
        self.logsdir = os.path.join('plots', self.RECOMMENDER_NAME, datetime.now().strftime("%Y%m%d-%H%M%S"))
        self.is_experiment = is_experiment
        if not self.is_experiment:
            os.makedirs(self.logsdir, exist_ok=True)
        self.items_to_ignore_flag = False
        self.items_to_ignore_ID = np.array([], dtype=int)
        self.filterTopPop = False
        self.filterTopPop_ItemsID = np.array([], dtype=int)
        self.initial_weights = None     # optional {'D': [...], 'G': [...]} in tensor-id order (init_weights' layout)
        self.engine = None
        self.params = None
        self.sess = None
        self._stop_training = False
        self.train_d_loss, self.train_g_loss = [], []

    # ---- engine plumbing -----------------------------------------------------------------------
    def _names(self):
        d, g = [], []
        for l in range(self.d_layers):
            d += ['discriminator/D_hidden_%d/kernel' % l, 'discriminator/D_hidden_%d/bias' % l]
        d += ['discriminator/D_output/kernel', 'discriminator/D_output/bias']
        for l in range(self.g_layers):
            g += ['generator/G_hidden_%d/kernel' % l, 'generator/G_hidden_%d/bias' % l]
        g += ['generator/G_output/kernel', 'generator/G_output/bias']
        return d, g

    def _get(self, tid):
        a = self.engine.get_tensor(tid)
        return a.reshape(-1) if (tid % 2 == 1) else a      # biases are 1-D in the reference

    def _build(self, d_nodes, d_layers, g_nodes, g_layers, d_hidden_act, g_hidden_act, scheme='ZR', d_batch_size=32, g_batch_size=32,
               zr_ratio=0., zr_coefficient=0., d_lr=1e-5, g_lr=1e-5, d_reg=0., g_reg=0.):
        from .engine import Engine
        for act in (d_hidden_act, g_hidden_act):
            if act not in L.ACT:
                raise ValueError("unknown or unsupported activation %r (supported: %s)" % (act, ", ".join(sorted(L.ACT))))
        if scheme not in SCHEMES:
            raise ValueError("scheme must be one of %r, given %r" % (SCHEMES, scheme))
        if d_layers < 1 or g_layers < 1:
            raise ValueError("CFGAN needs d_layers >= 1 and g_layers >= 1")
        self.d_nodes, self.d_layers, self.g_nodes, self.g_layers = d_nodes, d_layers, g_nodes, g_layers
        self.d_hidden_act, self.g_hidden_act, self.scheme, self.zr_ratio = d_hidden_act, g_hidden_act, scheme, zr_ratio
        if self.engine is not None:
            self.engine.close()
        self.engine = Engine(self.num_users, self.num_items, 1, d_nodes, max(d_batch_size, g_batch_size), d_lr=d_lr, g_lr=g_lr,
                             d_reg=d_reg, g_reg=g_reg, m=0.0, recon_coefficient=0.0, model=L.MODEL_CFGAN, d_layers=d_layers,
                             d_act=d_hidden_act, device=self.device, mfma=self.mfma)
        self.engine.set_urm(self._URM_fit)
        self.engine.set_seen(self._URM_eval)
        lens = np.diff(self._URM_fit.indptr)
        k_rows = [mask_size(self.num_items - int(n), zr_ratio) for n in lens]
        self.engine.cfgan_init(g_nodes, g_layers, g_hidden_act, d_batch_size, g_batch_size, scheme, zr_coefficient, self.seed, k_rows)
        self._reset_score_filter()
        d, g = self._names()
        self.params = {'D': [_TensorRef(i, n) for i, n in enumerate(d)],
                       'G': [_TensorRef(L.T_CFGAN_G0 + i, n) for i, n in enumerate(g)]}
        self.sess = _SessionShim(self)

    def _init_weights(self):
        w = self.initial_weights
        if w is None:
            w = init_weights(self.seed, self.num_items, self.d_nodes, self.d_layers, self.g_nodes, self.g_layers)
        for key in ('D', 'G'):
            for ref, a in zip(self.params[key], w[key]):
                self.engine.set_tensor(ref.tid, np.asarray(a, dtype=np.float32))

    # ---- fit (CFGAN.py:112-329) -------------------------------------------------------------------
    def fit(self, d_nodes=32, g_nodes=32, d_layers=1, g_layers=1, scheme='ZR', d_hidden_act='linear',
            g_hidden_act='linear', epochs=300, d_lr=1e-5, g_lr=1e-5, d_reg=0, g_reg=0, d_steps=1, g_steps=1,
            d_batch_size=32, g_batch_size=32, zr_ratio=0., zp_ratio=0., zr_coefficient=0., allow_worse=5, freq=5,
            after=0, metrics=['MAP'], validation_evaluator=None, sample_every=None, validation_set=None):
        self.config = dict(locals())
        del self.config['self']
        self._build(d_nodes, d_layers, g_nodes, g_layers, d_hidden_act, g_hidden_act, scheme=scheme, d_batch_size=d_batch_size,
                    g_batch_size=g_batch_size, zr_ratio=zr_ratio, zr_coefficient=zr_coefficient, d_lr=d_lr, g_lr=g_lr, d_reg=d_reg,
                    g_reg=g_reg)
        self._init_weights()

        self._stop_training = False
        watcher = None
        if allow_worse is not None and validation_evaluator is not None:
            watcher = EarlyStoppingScheduler(self, evaluator=validation_evaluator, allow_worse=allow_worse, freq=freq,
                                             metrics=metrics, after=after)
        self.train_d_loss, self.train_g_loss = [], []
        if self.verbose:
            print('Starting training...')
        fit_t0 = window_t0 = time.time()
        epoch = 1
        free = non_interactions(self._URM_fit) if self.mask_sampler == "numpy" else None
        while not self._stop_training and epoch < epochs + 1:
            if self.mask_sampler == "numpy":
                self.upload_masks(*draw_masks_numpy(self._URM_fit, scheme, zr_ratio, free=free))
            d_losses, g_losses = self.engine.cfgan_epoch(epoch, d_steps, g_steps, draw=(self.mask_sampler == "device"))
            self.train_d_loss.append(np.mean(d_losses) if len(d_losses) else np.nan)
            self.train_g_loss.append(np.mean(g_losses) if len(g_losses) else np.nan)
            if validation_set is not None and sample_every is not None and epoch % sample_every == 0:
                elapsed = time.time() - window_t0
                print('Epoch : {:d}. Total: {:.2f} secs, {:.2f} secs/epoch.'.format(epoch, elapsed, elapsed / sample_every))
                print(self._in_eval_orientation(lambda: validation_evaluator.evaluateRecommender(self)[1]))
                window_t0 = time.time()
            if watcher is not None:
                self._in_eval_orientation(lambda: watcher(epoch))
                if self._stop_training:
                    print('Training stopped, epoch:', epoch)
            epoch += 1
        if self.verbose:
            print('Training took {:.2f} seconds'.format(time.time() - fit_t0))
        self.URM_train = self._URM_eval
        return epoch - 1 if self._stop_training else epoch

    def upload_masks(self, zr, pm):
        """bool [rows, I] planes (draw_masks_numpy's) -> the device"""
        self.engine.cfgan_set_masks(pack_mask_rows(zr), pack_mask_rows(pm))

    def _in_eval_orientation(self, call):
        self.URM_train = self._URM_eval
        try:
            return call()
        finally:
            self.URM_train = self._URM_fit

    # ---- hooks used by EarlyStoppingScheduler (CFGAN.py:331-340) --------------------------------
    def stop_fit(self):
        self._stop_training = True

    def save_current_model(self):
        self.engine.snapshot_best()

    def load_model(self):
        self.engine.restore_best()

    def _require_engine(self):
        if self.engine is None:
            raise RuntimeError("CFGAN: model has no device state; call fit() or load_bundle() first")

    # ---- persistence (CFGAN.py:370-372) -----------------------------------------------------------
    def saveModel(self, folder_path, file_name):
        from .tf_bundle import write_bundle
        self._require_engine()
        os.makedirs(folder_path, exist_ok=True)
        write_bundle(os.path.join(folder_path, file_name),
                     {ref.name: self.sess.run(ref) for ref in self.params['D'] + self.params['G']})

    def load_bundle(self, folder_path, file_name, d_hidden_act='linear', g_hidden_act='linear'):
        """Inverse of saveModel: widths and depths are read from the bundle's shapes; the activations are not stored in it."""
        from .tf_bundle import read_bundle
        data = read_bundle(os.path.join(folder_path, file_name))
        d_layers = len([k for k in data if k.startswith('discriminator/D_hidden_') and k.endswith('/kernel')])
        g_layers = len([k for k in data if k.startswith('generator/G_hidden_') and k.endswith('/kernel')])
        d_nodes = data['discriminator/D_output/kernel'].shape[0]
        g_nodes = data['generator/G_output/kernel'].shape[0]
        self._build(d_nodes, d_layers, g_nodes, g_layers, d_hidden_act, g_hidden_act)
        for ref in self.params['D'] + self.params['G']:
            if ref.name not in data:
                raise KeyError("%s: checkpoint has no tensor %r" % (self.RECOMMENDER_NAME, ref.name))
            self.engine.set_tensor(ref.tid, data[ref.name])
        self.URM_train = self._URM_eval
