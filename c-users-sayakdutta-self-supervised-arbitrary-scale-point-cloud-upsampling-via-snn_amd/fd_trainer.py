"""Training driver for fd — the reference's ``fd/trainer.py`` ``Trainer`` (methods and return values) over
``TrainableSNNDistanceEstimation`` (sapcu_amd/fd_train.py).  With the optional ``grad_clip`` / ``grad_clip_type``, applied between
backward and step, ``train_step.run_epoch(trainer, loader, clamp_parameters=True)`` is the batch loop of the reference's
trainfd.py:264-313 in f32.  ``SyntheticFdPatches`` stands in for the reference's h5 distance-field data, absent here.

There is one eager step, ``Trainer.train_step``, written over the hooks of sapcu_amd/train_step.py.  ``Trainer`` runs it in f32 and
refuses ``use_amp`` / ``scaler`` / ``gradient_accumulation``; ``AmpTrainer`` is the reference's default configuration (config/fd.yaml
``use_amp: true``, trainfd.py:194-291): bf16 GEMMs, an optional GradScaler, gradient accumulation, and the EdgeConv form of blocks 1-3.

``GraphedTrainStep`` (train_step's, importable from here) replays one whole step of either trainer as a HIP graph and leaves
exactly the state the eager step leaves.

Not built, and the constructors say so: DataParallel (``model.module``), ``use_snn_decoder=True`` (refused by the model)."""
import contextlib

import numpy as np
import torch

from .train_step import GraphedTrainStep, TrainerHooks, finish_step  # noqa: F401 (GraphedTrainStep is public here)


class Trainer(TrainerHooks):
    BAD_INDEX_ERROR = "fd training step: %d neighbour indices outside their patch reached the EdgeConv backward"

    def __init__(self, model, optimizer, device=None, input_type='pointcloud', vis_dir=None, threshold=0.5, eval_sample=False,
                 grad_clip=None, grad_clip_type='norm', use_amp=False, scaler=None, gradient_accumulation=1):
        if use_amp or scaler is not None:
            raise NotImplementedError("fd_trainer.Trainer runs in f32: bf16 / GradScaler are AmpTrainer's")
        if gradient_accumulation != 1:
            raise NotImplementedError("fd_trainer.Trainer: gradient accumulation is AmpTrainer's")
        if hasattr(model, 'module'):
            raise NotImplementedError("fd training: DataParallel is not built (one process per GPU)")
        if grad_clip_type not in ('norm', 'value'):
            raise ValueError("grad_clip_type must be 'norm' or 'value'")
        self.model, self.optimizer, self.device = model, optimizer, device
        self.input_type, self.vis_dir, self.threshold, self.eval_sample = input_type, vis_dir, threshold, eval_sample
        self.grad_clip, self.grad_clip_type = grad_clip, grad_clip_type
        self.use_amp, self.scaler, self.gradient_accumulation, self.accumulation_step = False, None, 1, 0
        if device is not None:
            self.model.to(device)

    def _batch(self, data):
        x = data.get('input').to(self.device).float()
        gt = data.get('len').to(self.device).float()
        if gt.dim() in (2, 3) and gt.shape[-1] == 1 and gt.dim() == x.dim() - 1:        # [B, 1] / [B, N, 1] (fd/trainer.py:75-78)
            gt = gt.squeeze(-1)
        return x, gt

    def _begin(self, x, gt):
        if self.accumulation_step == 0:
            self.optimizer.zero_grad()
        self.accumulation_step += 1

    def _prepare(self):
        self.reset_model_states()

    def _loss(self, x, gt):
        """``model.compute_loss`` (fd/snn_coder.py:873-887) without its ``.item()``."""
        from . import fd_train
        loss = fd_train.distance_loss(self.model(x), gt)
        return loss, {'total_loss': loss.detach(), 'distance_loss': loss.detach()}, [("WARNING: NaN/Inf in loss value", torch.isfinite(loss))]

    def _bad_index_counter(self, device):
        from . import fd_train
        return fd_train.bad_index_counter(device)

    def _finish(self, update=None):
        # trainfd.py:286-288, 301-302: clips only for grad_clip > 0; a scaler in use is un-scaled either way
        return finish_step(self, unscale=True, clip=self.grad_clip is not None and self.grad_clip > 0, update=update)

    def train_step(self, data):
        """fd/trainer.py:24-36 with the options of trainfd.py:264-302 -> (loss value, loss dict); (None, None) when the loss or a
        gradient is not finite (gradients zeroed, the accumulation counter reset, as trainfd.py's except branch skips the batch);
        RuntimeError when a neighbour index outside its patch reached an EdgeConv backward.  ``Trainer`` runs it in f32 (in whatever
        arithmetic is set) with no scaler and a step per call; ``AmpTrainer`` sets the rest."""
        from . import fd_train
        self.model.train()
        x, gt = self._batch(data)
        self._begin(x, gt)
        self._prepare()
        fd_train.take_bad_index_count()
        amp = self.use_amp and self.scaler is not None
        with self._arithmetic():                                                   # forward AND backward
            loss, scalars, tests = self._loss(x, gt)
            for text, ok in tests:
                if not bool(ok):
                    print(text)
                    return self._abort()
            scaled = loss / self.gradient_accumulation if self.gradient_accumulation != 1 else loss
            (self.scaler.scale(scaled) if amp else scaled).backward()
        bad = fd_train.take_bad_index_count()
        if bad:
            self._abort()
            raise RuntimeError(self.BAD_INDEX_ERROR % bad)
        if self.accumulation_step % self.gradient_accumulation == 0 and not self._finish():
            return None, None
        values = {name: v.item() for name, v in scalars.items()}
        return values['total_loss'], values

    def evaluate(self, val_loader, return_metrics=False):
        """Mean loss over the loader's batches (0.0 for an empty loader); with return_metrics also the per-key batch means of
        ``calculate_metrics``."""
        self.model.eval()
        self.reset_model_states()
        per_batch = [self.eval_step_with_metrics(batch) for batch in val_loader]
        n = len(per_batch)
        mean_loss = sum(float(loss) for loss, _ in per_batch) / n if n else 0.0
        if not return_metrics:
            return mean_loss
        keys = sorted({key for _, m in per_batch for key in m})
        return mean_loss, {key: sum(m.get(key, 0.0) for _, m in per_batch) / n for key in keys}

    def eval_step(self, data):
        self.model.eval()
        return self.eval_step_with_metrics(data, metrics=False)[0]

    def eval_step_with_metrics(self, data, metrics=True):
        """-> (loss tensor, metrics dict) of one batch in whatever mode the model is in (the reference's method does not switch it)."""
        x, gt = self._batch(data)
        with torch.no_grad():
            pred = self.model(x)
            loss, loss_dict = self.model.compute_loss(pred, gt)
            return loss, (self.calculate_metrics(pred, gt, loss_dict) if metrics else loss_dict)

    def compute_loss(self, data):
        return self.compute_loss_with_dict(data)[0]

    def compute_loss_with_dict(self, data):
        x, gt = self._batch(data)
        return self.model.compute_loss(self.model(x), gt)

    @staticmethod
    def calculate_metrics(pred_distances, gt_distances, loss_dict):
        """The loss dict plus 'mae', 'mse' and 'relative_error' = mean(|pred - gt| / (gt + 1e-8)); one device-to-host copy."""
        err = (pred_distances - gt_distances).abs()
        mae, mse, rel = torch.stack([err.mean(), (err * err).mean(), (err / (gt_distances + 1e-8)).mean()]).tolist()
        return dict(loss_dict, mae=mae, mse=mse, relative_error=rel)

    def predict(self, data, return_uncertainty=False):
        if return_uncertainty:
            raise NotImplementedError("the distance decoder has no uncertainty output (the reference's branch expects a model "
                                      "that returns a pair)")
        self.model.eval()
        self.reset_model_states()
        with torch.no_grad():
            return self.model(data.get('input').to(self.device).float())

    def save_model(self, path):
        """One file with the model's and the optimiser's state under the reference's two keys."""
        state = {'model_state_dict': self.model.state_dict(), 'optimizer_state_dict': self.optimizer.state_dict()}
        torch.save(state, path)

    def load_model(self, path):
        state = torch.load(path, map_location=self.device)
        self.model.load_state_dict(state['model_state_dict'], strict=True)
        self.optimizer.load_state_dict(state['optimizer_state_dict'])

    def get_learning_rate(self):
        return self.optimizer.param_groups[0]['lr']

    def set_learning_rate(self, lr):
        for group in self.optimizer.param_groups:
            group['lr'] = lr

    def reset_model_states(self):
        reset = getattr(self.model, 'reset_states', None)
        if reset is not None:
            reset()


class AmpTrainer(Trainer):
    """``Trainer`` with the options of the reference's default fd configuration (trainfd.py:194-291): its constructor, its settings
    and the arithmetic the step runs in; the step itself is ``Trainer.train_step``.  ``use_amp``: the GEMMs, data and weight gradients of the step on bf16 operands with f32
    accumulation (``train.gemm_precision``; BatchNorm statistics, neurons, softmax, loss and optimiser stay f32, as under autocast;
    block 0's xyz EdgeConvs form x_n - x_i in f32 first).  ``scaler``: a GradScaler, driven through scale / unscale_ / step / update
    when ``use_amp`` (bf16 needs no loss scaling; a reference script runs unchanged).  ``gradient_accumulation``: loss / n, clip and
    step on every n-th call.  ``edgeconv``: how blocks 1-3 run (``fd_train.edgeconv_form``); "factored" is the measured faster of
    the two in bf16."""

    def __init__(self, model, optimizer, device=None, input_type='pointcloud', vis_dir=None, threshold=0.5, eval_sample=False,
                 grad_clip=None, grad_clip_type='norm', use_amp=True, scaler=None, gradient_accumulation=1, edgeconv="factored"):
        super().__init__(model, optimizer, device=device, input_type=input_type, vis_dir=vis_dir, threshold=threshold,
                         eval_sample=eval_sample, grad_clip=grad_clip, grad_clip_type=grad_clip_type)
        if edgeconv not in ("feature", "factored"):
            raise ValueError("edgeconv must be 'feature' or 'factored'")
        if int(gradient_accumulation) < 1:
            raise ValueError("gradient_accumulation must be >= 1")
        self.use_amp, self.scaler, self.gradient_accumulation, self.edgeconv = bool(use_amp), scaler, int(gradient_accumulation), edgeconv

    def _arithmetic(self):
        from . import fd_train
        from . import train as T
        stack = contextlib.ExitStack()
        stack.enter_context(T.gemm_precision("bf16" if self.use_amp else "f32"))
        stack.enter_context(fd_train.edgeconv_form(self.edgeconv))
        return stack


def rotation_to_x(normal):
    """The rotation that takes unit vector `normal` to (1, 0, 0) (Rodrigues; identity when they already agree), the alignment the
    reference's Subsamplerfd applies to every patch (fd/transform.py:55-57)."""
    a = np.asarray(normal, np.float64)
    a = a / np.linalg.norm(a)
    b = np.array([1.0, 0.0, 0.0])
    v = np.cross(a, b)
    s2 = float(v @ v)
    if s2 == 0.0:
        return np.eye(3)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + K + K @ K * ((1.0 - float(a @ b)) / s2)


class SyntheticFdPatches(object):
    """Stand-in for the reference's fd training loader (fd/datacore.py + Subsamplerfd; config/fd.yaml: 16 patches of 100 points per
    cloud): batches {'input': [B, N, M, 3] f32, 'len': [B, N] f32, 'seed': [B, N, 3] f64, 'shape': B names}.  Each cloud is 2048
    points on an analytic sphere (radius 0.5) or torus (R = 0.35, r = 0.15) shell in a random pose; a seed sits at a known
    distance `len` outside the surface along the normal of its foot point; its patch is the M nearest cloud points minus the
    seed, rotated normal -> x.  Deterministic in (seed, batch index)."""

    SPHERE_R, TORUS_R, TORUS_r = 0.5, 0.35, 0.15

    def __init__(self, batches, batch_size=4, patches=16, points=100, seed=0, cloud_points=2048, band=(0.005, 0.03)):
        self.batches, self.batch_size, self.patches, self.points = batches, batch_size, patches, points
        self.seed, self.cloud_points, self.band = seed, cloud_points, band

    def __len__(self):
        return self.batches

    @classmethod
    def surface_distance(cls, shape, pose, points):
        """Analytic distance of world-space `points` [.., 3] to the surface of `shape` posed by the orthogonal matrix `pose`."""
        q = np.asarray(points, np.float64) @ pose                 # back to the shape's frame (pose^-1 = pose^T; row vectors)
        if shape == "sphere":
            return np.abs(np.linalg.norm(q, axis=-1) - cls.SPHERE_R)
        ring = np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - cls.TORUS_R
        return np.abs(np.sqrt(ring ** 2 + q[..., 2] ** 2) - cls.TORUS_r)

    def _surface(self, rng, shape, n):
        if shape == "sphere":
            nrm = rng.normal(size=(n, 3))
            nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            return nrm * self.SPHERE_R, nrm
        u, v = rng.uniform(0, 2 * np.pi, (2, n))
        R, r = self.TORUS_R, self.TORUS_r
        pts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], 1)
        nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
        return pts, nrm

    def _cloud(self, rng):
        shape = "sphere" if rng.random() < 0.5 else "torus"
        pose, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        cloud, _ = self._surface(rng, shape, self.cloud_points)
        foot, nrm = self._surface(rng, shape, self.patches)
        d = rng.uniform(self.band[0], self.band[1], self.patches)
        seeds = foot + d[:, None] * nrm                           # outside, closer to its foot point than any curvature radius
        cloud, seeds, nrm = cloud @ pose.T, seeds @ pose.T, nrm @ pose.T
        dist = ((seeds[:, None, :] - cloud[None, :, :]) ** 2).sum(-1)
        idx = np.argsort(dist, axis=1, kind="stable")[:, :self.points]
        patches = cloud[idx] - seeds[:, None, :]
        for i in range(self.patches):
            patches[i] = patches[i] @ rotation_to_x(nrm[i]).T
        return patches.astype(np.float32), d.astype(np.float32), seeds, shape, pose

    def __iter__(self):
        for b in range(self.batches):
            rng = np.random.default_rng([self.seed, b])
            clouds = [self._cloud(rng) for _ in range(self.batch_size)]
            yield {"input": torch.from_numpy(np.stack([c[0] for c in clouds])), "len": torch.from_numpy(np.stack([c[1] for c in clouds])),
                   "seed": torch.from_numpy(np.stack([c[2] for c in clouds])), "shape": [c[3] for c in clouds],
                   "pose": torch.from_numpy(np.stack([c[4] for c in clouds]))}
