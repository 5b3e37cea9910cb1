"""A dataset as the trainer's data source (the protocol of lib/trainers/phase_trainer.py): batches(batch, g, device), faces,
faces_to_labels, length.

Order.  Position p = g * batch + i, epoch e = p // length, item = perm(seed, e)[p % length] (the identity without shuffle): a pure
function of (seed, batch, g), so a resumed run and every rank need no state.  Every `length` consecutive positions hold every item
once; the trainer asks rank r of `world` for g = s * world + r, so the ranks of a step are disjoint.  Unlike the reference's
DistributedSampler + DataLoader(drop_last=True), nothing is dropped at the end of an epoch: a batch that straddles two epochs takes
its tail from the next permutation.

Host side.  Threads only (min(num_workers, 16) of them, never sized from the CPU count; PIL's decoder releases the GIL): a worker
decodes one item (dataset.raw) and copies its bytes into its row of a pinned uint8 staging buffer.  Workers never touch the GPU and
never allocate pinned memory; the caller's thread hands them their buffer, and it issues the non-blocking copies, one `ingest` per
distinct source size of the batch and conditions.smpl_conditions.  A staging buffer goes back to the workers only after the event
recorded behind its copy has completed.  After serving g the source schedules g + stride .. g + prefetch * stride; a request that
was not prefetched is loaded the same way, synchronously, and gives the same bytes.  On a CPU device the same class runs
ingest_torch and preprocess_smpl_fix_body.
"""
import concurrent.futures as cf
import time

import numpy as np
import torch

from . import conditions
from .ingest import ingest, ingest_torch

MAX_THREADS = 16


def epoch_permutation(length, seed, epoch, shuffle=True):
    if not shuffle:
        return torch.arange(length)
    g = torch.Generator().manual_seed((int(seed) * 1_000_003 + int(epoch)) % (2 ** 63 - 1))
    return torch.randperm(length, generator=g)


class _Slot:
    """pinned staging for `n` items of one source size; `event` is recorded behind the last copy issued from it"""

    def __init__(self, n, shape):
        Hs, Ws = shape
        self.n, self.shape, self.event = n, shape, None
        self.rgb = torch.empty(n, Hs, Ws, 3, dtype=torch.uint8).pin_memory()
        self.mask = torch.empty(n, Hs, Ws, dtype=torch.uint8).pin_memory()
        self.seg = torch.empty(n, Hs, Ws, dtype=torch.uint8).pin_memory()
        self.views = (self.rgb.numpy(), self.mask.numpy(), self.seg.numpy())

    def free(self):
        return self.event is None or self.event.query()


class _Request:
    def __init__(self, indices, slot, futures):
        self.indices, self.slot, self.futures = indices, slot, futures


class DatasetTrainingSource:
    """DatasetTrainingSource(dataset, seed=0, stride=1, num_workers=4, prefetch=2, shuffle=True).  `dataset`: a
    lib/data/datasets.SHHQDataset (raw(i), faces, faces_to_labels, lbs_weights, template, joints, height, width, geo_only).
    batches() returns every key of synthetic.SyntheticTrainingSource.batches plus `masks` (and `latents` when the dataset has
    them).  fused=False runs ingest_torch on the device instead of the kernel."""

    def __init__(self, dataset, seed=0, stride=1, num_workers=4, prefetch=2, shuffle=True, fused=True):
        self.dataset, self.seed, self.stride, self.prefetch, self.shuffle = dataset, int(seed), max(1, int(stride)), max(0, int(prefetch)), bool(shuffle)
        self.fused = bool(fused)
        self.length = len(dataset)
        if self.length < 1:
            raise ValueError("DatasetTrainingSource: the dataset is empty")
        self.faces, self.faces_to_labels = dataset.faces, dataset.faces_to_labels
        self.num_workers = max(1, min(int(num_workers), MAX_THREADS))
        self._pool = cf.ThreadPoolExecutor(max_workers=self.num_workers, thread_name_prefix="dataset-source")
        self._pending, self._slots, self._perms, self._model = {}, [], {}, {}
        self._shape = None                      # the source size seen last: what a prefetched request's staging is sized for
        self.host_seconds = 0.0                 # time spent inside batches() on the caller's thread (tools/ingest_bench.py)

    # ---- order
    def indices(self, batch, g):
        out = []
        for i in range(int(batch)):
            p = int(g) * int(batch) + i
            e = p // self.length
            if e not in self._perms:
                if len(self._perms) > 4:
                    self._perms.clear()
                self._perms[e] = epoch_permutation(self.length, self.seed, e, self.shuffle).tolist()
            out.append(self._perms[e][p % self.length])
        return out

    # ---- host side
    def _load(self, index, slot, row):
        try:
            raw = self.dataset.raw(index)
        except Exception as e:
            raise RuntimeError(f"DatasetTrainingSource: loading item {index} of {getattr(self.dataset, 'root', '?')} failed: "
                               f"{type(e).__name__}: {e}") from e
        if slot is not None and raw["rgb"].shape[:2] == slot.shape:
            for view, key in zip(slot.views, ("rgb", "mask", "seg")):
                np.copyto(view[row], raw.pop(key))
            raw["staged"] = True
        return raw

    def _acquire(self, n, shape):
        """a free staging buffer for n items of `shape` (caller's thread only)"""
        for s in self._slots:
            if s.n == n and s.shape == shape and s.free():
                self._slots.remove(s)
                s.event = None
                return s
        return _Slot(n, shape)

    def _release(self, slot):
        if len(self._slots) < 2 * (self.prefetch + 2):
            self._slots.append(slot)

    def _schedule(self, batch, g, cuda):
        idx = self.indices(batch, g)
        slot = self._acquire(batch, self._shape) if (cuda and self._shape is not None) else None
        return _Request(idx, slot, [self._pool.submit(self._load, i, slot, row) for row, i in enumerate(idx)])

    def _drop(self, req):
        for f in req.futures:
            f.cancel()
        cf.wait(req.futures)
        if req.slot is not None:
            self._release(req.slot)

    def close(self):
        """stop the pool; pending requests are dropped"""
        for req in self._pending.values():
            for f in req.futures:
                f.cancel()
        self._pending.clear()
        self._pool.shutdown(wait=True)
        self._slots.clear()

    def __del__(self):
        try:
            self._pool.shutdown(wait=False)
        except Exception:
            pass

    # ---- the caller's thread
    def _to_device(self, req, raws, rows, shape, device):
        """the uint8 tensors of the items `rows` (all of source size `shape`) on `device`"""
        if device.type != "cuda":
            stack = lambda k: torch.from_numpy(np.stack([raws[r][k] for r in rows]))                    # noqa: E731
            return stack("rgb"), stack("mask"), stack("seg")
        if req.slot is not None and rows == list(range(req.slot.n)) and all(raws[r].get("staged") for r in rows):
            slot = req.slot
            req.slot = None
        else:
            slot = self._acquire(len(rows), shape)
            for j, r in enumerate(rows):                # a first request, or a batch of several source sizes: staged here
                for k, key in enumerate(("rgb", "mask", "seg")):
                    np.copyto(slot.views[k][j], req.slot.views[k][r] if raws[r].get("staged") else raws[r][key])
        out = tuple(t.to(device, non_blocking=True) for t in (slot.rgb, slot.mask, slot.seg))
        slot.event = torch.cuda.Event()
        slot.event.record()
        self._release(slot)
        return out

    def _model_on(self, device):
        key = str(device)
        if key not in self._model:
            self._model[key] = (self.dataset.lbs_weights.to(device), self.dataset.template.to(device))
        return self._model[key]

    def _conditions(self, raws, device):
        ds = self.dataset
        if device.type != "cuda":
            items = [ds._conditions(r) for r in raws]
            cond = {k: torch.stack([it[k] for it in items]) for k in items[0]}
        else:
            host = {k: torch.from_numpy(np.concatenate([np.asarray(r[k], dtype=np.float32) for r in raws])) for k in
                    ("fk_matrices", "joints", "full_pose", "tpose_vertices")}
            cam = torch.from_numpy(np.concatenate([np.asarray(r["orig_cam"], dtype=np.float32).reshape(1, -1)[:, :4] for r in raws]))
            lbs, template = self._model_on(device)
            smpl_out = {k: v.to(device, non_blocking=True) for k, v in host.items()}
            smpl_out["lbs_weights"] = lbs
            cond = conditions.smpl_conditions(smpl_out, cam.to(device, non_blocking=True), ds.joints, template)
            if ds.inference:
                cond["body_shape"] = torch.from_numpy(np.concatenate([np.asarray(r["betas"], dtype=np.float32) for r in raws])).to(device)
        zero = torch.zeros(len(raws))
        cond["cam2world_matrices"] = conditions.CameraPreprocessor(device).forward_with_rotation(cond, zero, zero, zero)["cam2world_matrices"]
        return cond

    def batches(self, batch, g, device):
        t0 = time.perf_counter()
        batch, g, device = int(batch), int(g), torch.device(device)
        cuda = device.type == "cuda"
        req = self._pending.pop((batch, g), None)
        if req is None:
            req = self._schedule(batch, g, cuda)
        try:
            raws = [f.result() for f in req.futures]
        except BaseException:
            self._drop(req)
            raise
        size = (self.dataset.height, self.dataset.width)
        groups = {}
        for row, r in enumerate(raws):
            shape = tuple(req.slot.shape) if r.get("staged") else tuple(r["rgb"].shape[:2])
            groups.setdefault(shape, []).append(row)
        self._shape = next(iter(groups))
        run = ingest if (cuda and self.fused) else ingest_torch
        parts = []
        for shape, rows in groups.items():
            parts.append((rows, run(*self._to_device(req, raws, rows, shape, device), size, self.dataset.geo_only)))
        if req.slot is not None:                # nothing was copied from it: free at once
            self._release(req.slot)
        if len(parts) == 1:
            out = dict(parts[0][1])
        else:
            out = {}
            for k in parts[0][1]:
                first = parts[0][1][k]
                full = torch.empty((batch,) + tuple(first.shape[1:]), dtype=first.dtype, device=first.device)
                for rows, res in parts:
                    full[torch.as_tensor(rows, device=first.device)] = res[k]
                out[k] = full
        out.update(self._conditions(raws, device))
        out["indices"] = torch.as_tensor([r["index"] for r in raws]).to(device)
        if all("latent" in r for r in raws):
            out["latents"] = torch.from_numpy(np.stack([r["latent"] for r in raws])).to(device)
        # look ahead; requests nobody came back for are dropped, oldest first
        for k in range(1, self.prefetch + 1):
            key = (batch, g + k * self.stride)
            if key not in self._pending:
                self._pending[key] = self._schedule(batch, key[1], cuda)
        while len(self._pending) > 2 * max(self.prefetch, 1):
            self._drop(self._pending.pop(next(iter(self._pending))))
        self.host_seconds += time.perf_counter() - t0
        return out
