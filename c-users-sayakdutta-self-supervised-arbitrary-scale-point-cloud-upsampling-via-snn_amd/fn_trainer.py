"""Training driver for fn — the reference's ``fn/trainer.py`` ``Trainer`` (:9-148 train_step, :150-227 evaluate, :229-247
eval_step) over the HIP training ops of sapcu_amd/train.py.  Same constructor arguments, same return values, same
skip-the-batch behaviour on NaN/Inf.  The optimiser is whatever torch optimiser the caller built on model.parameters()
(the reference's trainfn.py:107-109 builds AdamW/Adam).  ``use_amp=True`` runs the Conv / Linear GEMMs of the step — forward,
data gradient, weight gradient — on bf16 operands with f32 accumulation (sapcu_amd.train.gemm_precision, csrc/train_bf16.hip):
the counterpart of the reference's ``torch.amp.autocast`` region (fn/trainer.py:67-83; BASELINE config 5 names bf16, whose f32
exponent range needs no loss scaling — a GradScaler, if given, is still driven through scale / unscale_ / step / update so a
reference training script runs unchanged).  The step is written over the hooks of sapcu_amd/train_step.py, which also holds what
fn shares with fd and keeps importable from here: the step's tail, ``run_epoch`` (the batch loop of trainfn.py:253-330),
``clamp_neuron_parameters`` and ``GraphedTrainStep`` (the step replayed as one HIP graph, equal to this one bit for bit).
``SyntheticPU1K`` stands in for the PU1K mesh sampler (fn/datacore.py needs trimesh and the meshes, absent here)."""
import numpy as np
import torch
from torch.nn import functional as F

from .train_step import GraphedTrainStep, TrainerHooks, clamp_neuron_parameters, finish_step, run_epoch  # noqa: F401 (public here)


class Trainer(TrainerHooks):
    def __init__(self, model, optimizer, device=None, input_type='pointcloud', vis_dir=None, threshold=0.5, eval_sample=False,
                 gradient_accumulation=1, use_amp=False, scaler=None, grad_clip=None, grad_clip_type='norm'):
        self.model, self.optimizer, self.device = model, optimizer, device
        self.input_type, self.vis_dir, self.threshold, self.eval_sample = input_type, vis_dir, threshold, eval_sample
        self.gradient_accumulation = gradient_accumulation
        self.use_amp, self.scaler = use_amp, scaler
        self.grad_clip, self.grad_clip_type = grad_clip, grad_clip_type
        self.accumulation_step = 0
        if device is not None:
            self.model.to(device)

    def _batch(self, data):
        dd = {k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in data.items()}
        return dd['input'].float(), dd['normal'].float()

    @staticmethod
    def _finite(t):
        return bool(torch.isfinite(t).all())

    def _begin(self, points, gt):
        """fn/trainer.py:43-61: the batch is counted, then refused when its input or target is not finite (one sync for both)."""
        self.accumulation_step += 1
        if not bool(torch.stack([torch.isfinite(points).all(), torch.isfinite(gt).all()]).all()):
            return "WARNING: NaN/Inf detected in the batch at step %d" % self.accumulation_step
        return None

    def _arithmetic(self):
        from . import train as T
        return T.gemm_precision("bf16" if self.use_amp else "f32")       # forward and backward, like the autocast region + backward

    def _loss(self, points, gt):
        """``model.compute_loss`` (fn/snn_coder.py:701-724) on the normalised prediction and target without its two ``.item()``."""
        from . import train as T
        pred = self.model(points)
        tests = [("WARNING: NaN/Inf in model predictions", torch.isfinite(pred).all())]
        xyz = points.mean(dim=2) if points.ndim == 4 else points
        loss, conf = T.angular_loss_with_consistency(F.normalize(pred, dim=-1), F.normalize(gt, dim=-1), xyz)
        tests.append(("WARNING: NaN/Inf in loss value", torch.isfinite(loss).all()))
        return loss, {"total_loss": loss.detach(), "confidence": conf.detach()}, tests

    def _finish(self, update=None):
        clip = self.grad_clip is not None                                 # fn/trainer.py:101-108: clips whenever a bound is set, un-scales only then
        return finish_step(self, unscale=clip, clip=clip, update=update)

    def _skip(self):
        return None, None                                                 # fn/trainer.py:69-96: these returns leave the accumulation counter as it is

    def train_step(self, data):
        """One optimisation step (fn/trainer.py:41-148): -> (loss value, loss dict), or (None, None) for a skipped batch."""
        self.model.train()
        points, gt = self._batch(data)
        warning = self._begin(points, gt)
        if warning is not None:
            print(warning)
            return None, None
        amp = self.use_amp and self.scaler is not None
        with self._arithmetic():
            loss, scalars, tests = self._loss(points, gt)
            for text, ok in tests:
                if not bool(ok):
                    print(text)
                    return self._skip()
            scaled = loss / self.gradient_accumulation
            (self.scaler.scale(scaled) if amp else scaled).backward()
        if self.accumulation_step % self.gradient_accumulation == 0 and not self._finish():
            return None, None
        values = {name: v.item() for name, v in scalars.items()}
        return values["total_loss"], values

    @staticmethod
    def compute_angular_error(pred, gt):
        cos = torch.clamp(F.cosine_similarity(pred, gt, dim=-1), -1 + 1e-6, 1 - 1e-6)
        return torch.rad2deg(torch.acos(cos)).mean()

    cos_sim = compute_angular_error

    def eval_step(self, data):
        self.model.eval()
        points, gt = self._batch(data)
        with torch.no_grad():
            pred = self.model(points)
            loss, loss_dict = self.model.compute_loss(pred, gt, points)
        return loss.item(), (loss_dict or {}).get('confidence', 0.0)

    def evaluate(self, val_loader):
        """fn/trainer.py:150-227: -> (mean loss, mean confidence, {'confidence', 'angular_error_deg'})."""
        self.model.eval()
        total_loss = total_conf = total_err = 0.0
        batches, confs, errs = 0, [], []
        with torch.no_grad():
            for data in val_loader:
                points, gt = self._batch(data)
                if not self._finite(points):
                    print("WARNING: NaN/Inf in validation input, skipping batch")
                    continue
                gt = F.normalize(gt, dim=-1)
                pred = F.normalize(self.model(points), dim=-1)
                loss, loss_dict = self.model.compute_loss(pred, gt, points)
                if not self._finite(loss):
                    print("WARNING: NaN/Inf in validation loss, skipping batch")
                    continue
                err = self.compute_angular_error(pred.reshape(-1, 3), gt.reshape(-1, 3)).item()
                total_loss += loss.item()
                total_err += err
                total_conf += loss_dict['confidence']
                confs.append(loss_dict['confidence'])
                errs.append(err)
                batches += 1
        n = max(batches, 1)
        metrics = {}
        if confs:
            metrics['confidence'] = float(np.mean(confs))
        metrics['angular_error_deg'] = total_err / n
        return total_loss / n, total_conf / n, metrics


class SyntheticPU1K(object):
    """Stand-in for the reference's PU1K training loader (fn/datacore.py; config/fn.yaml: batch_size 4, 64 patches of 12 points
    per cloud): batches {'input': [B, N, M, 3] f32 centred patches, 'normal': [B, N, 3] unit normals} sampled from analytic
    surfaces whose normals are known (sphere and torus shells, random pose), deterministic in (seed, batch index)."""

    def __init__(self, batches, batch_size=4, patches=64, points=12, seed=0, radius=0.06):
        self.batches, self.batch_size, self.patches, self.points, self.seed, self.radius = batches, batch_size, patches, points, seed, radius

    def __len__(self):
        return self.batches

    def _cloud(self, rng):
        n, m = self.patches, self.points
        c = rng.normal(size=(n, 3))
        c /= np.linalg.norm(c, axis=1, keepdims=True)                    # patch centres on a unit sphere ...
        nrm = c.copy()
        if rng.random() < 0.5:                                           # ... or on a torus (R = 0.7, r = 0.3): normals differ from positions
            u, v = rng.uniform(0, 2 * np.pi, (2, n))
            c = np.stack([(0.7 + 0.3 * np.cos(v)) * np.cos(u), (0.7 + 0.3 * np.cos(v)) * np.sin(u), 0.3 * np.sin(v)], 1)
            nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
        # tangent-plane samples around each centre, pushed back along the normal by the local curvature (1 / 2 x^2 term)
        t1 = np.cross(nrm, rng.normal(size=(n, 3)))
        t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
        t2 = np.cross(nrm, t1)
        ab = rng.uniform(-self.radius, self.radius, (n, m, 2))
        pts = ab[..., :1] * t1[:, None, :] + ab[..., 1:] * t2[:, None, :] - 0.5 * (ab ** 2).sum(-1, keepdims=True) * nrm[:, None, :]
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))                     # random pose of the whole cloud
        return (pts @ q.T).astype(np.float32), (nrm @ q.T).astype(np.float32)

    def __iter__(self):
        for b in range(self.batches):
            rng = np.random.default_rng([self.seed, b])
            clouds = [self._cloud(rng) for _ in range(self.batch_size)]
            yield {"input": torch.from_numpy(np.stack([c[0] for c in clouds])), "normal": torch.from_numpy(np.stack([c[1] for c in clouds]))}
