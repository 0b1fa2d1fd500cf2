"""Host-to-device input staging overlapped with the previous training / inference step.

The model boundary takes device tensors (`EMSANet.forward(batch)`); the reference's loop moves every
batch synchronously right before the step (`/root/reference/main.py:112-123`, timing protocol of
`/root/reference/inference_time_whole_model.py:297-347` includes that copy).  `BatchStager` is the
MI355X-side replacement for that copy:

  * the loader hands over RAW frames in pinned host memory -- uint8 RGB (N,H,W,3) and uint16 depth
    (N,H,W), 1-2 bytes per value instead of the 4 of the normalised float tensors (a bs=32 640x480
    RGB-D batch is 49 MB instead of 157 MB: 0.8 ms instead of 2.5 ms over PCIe);
  * batch i+1 is copied on a separate HIP stream into a ring of device buffers while step i runs;
  * `NormalizeRGB` / `NormalizeDepth` + HWC->CHW (`/root/reference/emsanet/preprocessing.py:216-226`)
    run as kernels on the compute stream (`postprocessing.normalize_*`) when the batch is handed
    out, so nothing but events crosses between the streams.
Float tensors in the incoming dict (already normalised inputs, targets) are staged as they are.
With a `target_generator` (`emsanet_amd.targets.TrainingTargetGenerator`) the loader ships the raw
'semantic' / 'instance' label maps (plus 'orientations', 'scene') and the training targets are
generated from the staged maps on the compute stream, under 'targets'.
With an `augmenter` (`emsanet_amd.augment.TrainingAugmenter`) the loader ships UN-AUGMENTED raw frames
and label maps: resize, crop, HSV jitter and flip run fused with the normalisation when the batch is
handed out, and the targets are generated from the augmented maps.
With a `decoder` (`emsanet_amd.png.PngDecoder`) the loader may ship a value as the PNG FILES themselves
(`emsanet_amd.png.PngFiles`): only the file bytes cross on the copy stream, and the files are decoded on
the compute stream when the batch is handed out, in front of everything above.
"""
from typing import Dict, Iterable, Iterator

import torch

from . import _lib
from . import functional as Fn
from .png import PngFiles
from .postprocessing import normalize_depth, normalize_rgb


class BatchStager:
    """iterate over `host_batches` (dicts of pinned CPU tensors), yield dicts of device tensors.

    depth_stats = (mean, std) of the depth normalisation; `ring` device buffer sets: a set is
    refilled (on the copy stream) as soon as the kernels that read its previous content have been
    enqueued.  Non-tensor entries of a batch are passed through.  target_generator: when given, its
    `generate` runs over the staged label maps of every batch and the result is handed out under
    'targets' (its own ring must be at least as deep as the number of batches the caller keeps).
    augmenter: when given, its `apply` runs over the staged raw buffers instead of the two
    normalisation kernels (it carries its own depth statistics); its outputs -- normalised inputs,
    augmented label maps, orientation table -- are handed out and feed the target generator.  The same
    holds for the depth of its ring.
    decoder: when given, a batch value that is a `PngFiles` has its file bytes and offsets table staged
    (`bytes_staged` counts the file bytes) and is decoded at hand-out into the decoder's own ring; the
    stack then takes the place of the raw frames.  `decoder.check()` stays the caller's (it synchronises)."""

    def __init__(self, host_batches: Iterable[Dict], device, depth_stats=(0.0, 1.0), ring: int = 2,
                 rgb_key: str = 'rgb', depth_key: str = 'depth', target_generator=None, augmenter=None,
                 decoder=None):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.EmsaError(f"BatchStager stages batches onto an AMD GPU, not onto {self.device}")
        if ring < 2:
            raise ValueError("ring must be >= 2 (one buffer set being drained, one being filled)")
        self.src = host_batches
        self.depth_stats = depth_stats
        self.ring = ring
        self.rgb_key, self.depth_key = rgb_key, depth_key
        self.target_generator = target_generator
        self.augmenter = augmenter
        self.decoder = decoder
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self._slots = [dict(bufs={}, copied=torch.cuda.Event(), freed=None) for _ in range(ring)]
        self.bytes_staged = 0
        self.batches_staged = 0

    # -- one slot: raw device buffers that the copy stream fills and the compute stream drains ----
    def _issue(self, slot, host_batch):
        slot['files'] = {}
        with torch.cuda.stream(self.copy_stream):
            if slot['freed'] is not None:
                # the buffers' previous content was consumed by kernels on the compute stream
                self.copy_stream.wait_event(slot['freed'])
            for k, v in host_batch.items():
                if isinstance(v, PngFiles):
                    slot['files'][k] = self._issue_files(slot, k, v)
                    continue
                if not torch.is_tensor(v):
                    continue
                if v.is_cuda:
                    slot['bufs'][k] = v
                    continue
                if not v.is_pinned():
                    raise _lib.EmsaError(f"batch['{k}'] is pageable host memory: the overlapped copy "
                                         "needs pinned memory (DataLoader(pin_memory=True))")
                buf = slot['bufs'].get(k)
                if buf is None or buf.shape != v.shape or buf.dtype != v.dtype:
                    buf = Fn._empty(v.shape, self.device, v.dtype)
                    slot['bufs'][k] = buf
                buf.copy_(v, non_blocking=True)
                self.bytes_staged += v.numel() * v.element_size()
            slot['copied'].record(self.copy_stream)
        slot['extra'] = {k: v for k, v in host_batch.items() if not (torch.is_tensor(v) or isinstance(v, PngFiles))}
        slot['keys'] = [k for k, v in host_batch.items() if torch.is_tensor(v) or isinstance(v, PngFiles)]
        self.batches_staged += 1

    def _issue_files(self, slot, k, files):
        """(on the copy stream) the file bytes and the offsets table of one PngFiles into the slot's byte
        buffer, which grows in powers of two -> the PngFiles over the device copies"""
        if self.decoder is None:
            raise _lib.EmsaError(f"batch['{k}'] is a PngFiles and the stager has no decoder: "
                                 "BatchStager(..., decoder=PngDecoder())")
        if files.data.is_cuda:
            return files
        if not (files.data.is_pinned() and files.offsets.is_pinned()):
            raise _lib.EmsaError(f"batch['{k}']: the files are in pageable host memory: the overlapped copy "
                                 "needs pinned memory (PngFiles.from_bytes pins)")
        name = ('png', k)
        buf = slot['bufs'].get(name)
        n = files.data.numel()
        if buf is None or buf[0].numel() < n or buf[1].numel() != files.m + 1:
            size = 1 << max(12, (n - 1).bit_length())
            buf = slot['bufs'][name] = (Fn._empty((size,), self.device, torch.uint8),
                                        Fn._empty((files.m + 1,), self.device, torch.int64))
        buf[0][:n].copy_(files.data, non_blocking=True)
        buf[1].copy_(files.offsets, non_blocking=True)
        self.bytes_staged += n
        return PngFiles(buf[0], buf[1], files.m, files.layout, files.h, files.w, files.file_bytes, n)

    def _hand_out(self, slot):
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(slot['copied'])
        out = dict(slot['extra'])
        bufs = slot['bufs']
        if slot['files']:
            # reads the file bytes on the compute stream: covered by the `freed` event below
            bufs = dict(bufs)
            bufs.update(self.decoder.decode_batch(slot['files']))
        augmented = {}
        if self.augmenter is not None:
            # reads the raw buffers on the compute stream: covered by the `freed` event below
            names = {self.rgb_key: 'rgb', self.depth_key: 'depth'}
            res = self.augmenter.apply({names.get(k, k): bufs[k] for k in slot['keys']})
            back = {'rgb': self.rgb_key, 'depth': self.depth_key}
            augmented = {back.get(k, k): v for k, v in res.items()}
        for k in slot['keys']:
            raw = bufs[k]
            if k in augmented:
                out[k] = augmented[k]
            elif k == self.rgb_key and raw.dtype == torch.uint8:
                out[k] = normalize_rgb(raw)
            elif k == self.depth_key and raw.dtype in (torch.uint16, torch.int16):
                out[k] = normalize_depth(raw, *self.depth_stats)
            else:
                # handed out as is: it must not be overwritten while the step uses it
                out[k] = raw.clone()
        if self.target_generator is not None:
            # reads the raw buffers on the compute stream: covered by the `freed` event below
            out['targets'] = self.target_generator.generate(
                {k: augmented.get(k, bufs[k]) for k in slot['keys']})
        ev = torch.cuda.Event()
        ev.record(cur)           # every reader of the raw buffers has been enqueued before this
        slot['freed'] = ev
        return out

    def __iter__(self) -> Iterator[Dict]:
        it = iter(self.src)
        pending = []                      # slots whose copies are in flight, oldest first
        free = list(self._slots)
        exhausted = False

        def top_up():
            nonlocal exhausted
            while free and not exhausted:
                try:
                    hb = next(it)
                except StopIteration:
                    exhausted = True
                    return
                s = free.pop(0)
                self._issue(s, hb)
                pending.append(s)

        top_up()
        while pending:
            s = pending.pop(0)
            batch = self._hand_out(s)
            free.append(s)
            top_up()                      # the next copy starts before the step's kernels are launched
            yield batch


def pinned_raw_batch(n: int, h: int, w: int, seed: int = 0, modalities=('rgb', 'depth')) -> Dict:
    """synthetic RAW frames in pinned host memory (uint8 RGB, uint16 depth in mm with ~5 % invalid
    pixels), the form a camera driver / decoded dataset sample has before preprocessing"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    if 'rgb' in modalities:
        out['rgb'] = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8).pin_memory()
    if 'depth' in modalities:
        d = torch.randint(300, 8000, (n, h, w), generator=g, dtype=torch.int32)
        d[torch.rand((n, h, w), generator=g) < 0.05] = 0
        out['depth'] = d.to(torch.uint16).pin_memory()
    return out
