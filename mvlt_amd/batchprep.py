"""Device-side batch preparation and prefetch.

In the reference every sample is masked on the host inside DataLoader workers -- `generate_grid_mask` +
`image.clone().masked_fill_(mask, 1e-6)` (mcloader/fashion_gen.py:167,176,225-254) and `random_masking_features`
(:383-409) -- and the engine then moves seven tensors per batch to the GPU (engine_grid_masking.py:42-56).  Here the loader
only has to deliver the clean image, the original token ids and the three small label tensors:

  DeviceBatchPrep   grid mask (exact-count or the reference's sliding-window generator), the 1e-6 fill, the 80/10/10 token
                    masking and the masked-index selection as HIP kernels (csrc/batchprep.hip) on a counter-based generator
                    (Philox4x32-10 keyed by seed, counted by sample id), bit-exact against oracle/batchprep_oracle.py
                    With uint8 input (what the loader DECODED: native-size pixels and one source rectangle per sample) the content crop, Resize,
                    ToTensor (+ Normalize) and a horizontal flip move to the device too, and the clean fp32 image and its masked copy come out of one
                    pass (csrc/ingest.hip, docs/ingest.md)
  DevicePrefetcher  the reference's DataPrefetcher idea (mcloader/data_prefetcher.py:4-28: copy the NEXT batch on a side stream
                    while the current one computes) for the engine's dict batches: pinned staging, H2D and the preparation
                    kernels on a side HIP stream, the MLM selection count brought back to the host on that stream too, so the
                    step that consumes the batch never waits for it (`mlm_count`, schedule.run_forward)

Both yield the batch-dict schema `train_one_epoch_vl` consumes.
"""
import torch

from . import ops

PATCH = 16                       # fashion_gen.py:167 patch_size=16
FILL = 1e-6                      # fashion_gen.py:176


class DeviceBatchPrep:
    def __init__(self, seed, mask_ratio=0.5, mode="exact", vocab=30522, hflip=0.0, mean=None, std=None, size=None):
        """mode "exact": exactly int(mask_ratio * patches) masked patches per image; "reference": the reference generator's
        sliding-window variant (realised ratio varies around mask_ratio).
        hflip / mean / std / size act on uint8 input only (docs/ingest.md): the probability of a horizontal flip per sample, the per-channel Normalize
        constants, and the output size (int or (H, W); None = the input's)."""
        assert mode in ("exact", "reference")
        assert 0.0 <= hflip <= 1.0 and (mean is None) == (std is None)
        self.seed, self.mask_ratio, self.mode, self.vocab = int(seed), float(mask_ratio), mode, vocab
        self.hflip, self.mean, self.std = float(hflip), mean, std
        self.size = (int(size), int(size)) if isinstance(size, int) else (None if size is None else (int(size[0]), int(size[1])))
        self.sample = 0                           # running sample id: sample b of a call is self.sample + b
        self._consts, self._whole = {}, {}        # per device: (value table, norm); per (device, B, h, w): the whole-slab rectangles (device, host)

    def __call__(self, image, ori_input_ids, sample0=None, select=True, rects=None, rects_host=None):
        """image (B,3,H,W) fp32 (H and W multiples of the 16-pixel patch, not necessarily equal) and ori_input_ids (B,T) int64 on the
        device -> dict(masked_images (B,3,H,W), patch_flags (B,H/16,W/16), input_ids, mlm_labels[, mlm_positions_buf, mlm_count_dev]);
        kernels go to torch's current stream.
        image uint8 (B,h,w,3): the dict also carries `image` (the clean fp32 (B,3,H,W) image) and `flip` (uint8 (B)); see `_ingest`."""
        assert image.is_cuda and image.dtype in (torch.float32, torch.uint8) and ori_input_ids.dtype == torch.int64
        ori = ori_input_ids.contiguous()
        if sample0 is None:
            sample0 = self.sample
            self.sample += image.shape[0]
        dev = image.device
        if image.dtype == torch.uint8:
            out = self._ingest(image, sample0, rects, rects_host)
        else:
            assert rects is None and rects_host is None, "rectangles go with uint8 input"
            assert image.dim() == 4 and image.shape[2] % PATCH == 0 and image.shape[3] % PATCH == 0, \
                f"image must be (B, 3, H, W) with H and W multiples of {PATCH}, got {tuple(image.shape)}"
            image = image.contiguous()
            B, C, H, W = image.shape
            flags = self._flags(B, H, W, sample0, dev)
            masked = torch.empty_like(image)
            ops.grid_mask_apply(image, flags, masked, PATCH, FILL)
            out = dict(masked_images=masked, patch_flags=flags.view(B, H // PATCH, W // PATCH))
        ids, labels = torch.empty_like(ori), torch.empty_like(ori)
        ops.token_mask(ori, ids, labels, self.seed, sample0, self.vocab)
        out.update(input_ids=ids, mlm_labels=labels)
        if select:
            idx = torch.empty(labels.numel(), device=dev, dtype=torch.int32)
            cnt = torch.zeros(1, device=dev, dtype=torch.int32)
            ops.masked_select(labels.view(-1), idx, cnt)
            out["mlm_positions_buf"], out["mlm_count_dev"] = idx, cnt
        return out

    def _flags(self, B, H, W, sample0, dev):
        gh, gw = H // PATCH, W // PATCH
        flags = torch.empty(B, gh * gw, dtype=torch.uint8, device=dev)
        ops.grid_mask_flags(flags, B, gh, gw, int(self.mask_ratio * gh * gw), 0 if self.mode == "exact" else 1, self.seed, sample0)
        return flags

    def _ingest(self, src, sample0, rects, rects_host):
        """uint8 (B,h,w,3) -> dict(image, masked_images, patch_flags, flip).  The flags are drawn first, so the masked copy comes out of the ingest pass itself:
        `grid_mask_apply` is not launched.  Without rectangles, with (h, w) equal to the output size and hflip == 0 the no-resample kernel runs (a table lookup per
        pixel); anything else takes the resize kernel, rectangles defaulting to the whole slab (at equal sizes its output is bit-identical to the lookup).
        rects: int32 (B,4) = (y0, x0, h, w), on the CPU (copied to the device here) or on the device together with rects_host, its CPU copy -- the entry point
        checks the host values before it launches; a device tensor alone is read back (a sync)."""
        assert src.dim() == 4 and src.shape[3] == 3, f"uint8 image must be (B, h, w, 3), got {tuple(src.shape)}"
        src, dev = src.contiguous(), src.device
        B, h, w, _ = src.shape
        H, W = self.size or (h, w)
        assert H % PATCH == 0 and W % PATCH == 0, f"the output size must be multiples of {PATCH}, got {(H, W)}"
        if dev not in self._consts:
            self._consts[dev] = (ops.ingest_table(self.mean, self.std).to(dev), None if self.mean is None else ops.ingest_norm(self.mean, self.std).to(dev))
        table, norm = self._consts[dev]
        flags = self._flags(B, H, W, sample0, dev)
        flip = ops.flip_flags(torch.empty(B, dtype=torch.uint8, device=dev), self.hflip, self.seed, sample0)
        image = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        masked = torch.empty_like(image)
        if rects is None and (h, w) == (H, W) and self.hflip == 0.0:
            ops.image_ingest(src, table, image, masked, flags, 0, PATCH, FILL)
        else:
            if rects is None:
                key = (dev, B, h, w)
                if key not in self._whole:
                    host = torch.tensor([[0, 0, h, w]] * B, dtype=torch.int32)
                    self._whole[key] = (host.to(dev), host)
                rects, rects_host = self._whole[key]
            elif not rects.is_cuda:
                rects_host = rects.to(torch.int32).contiguous()
                rects = rects_host.to(dev, non_blocking=True)
            else:
                rects = rects.to(torch.int32).contiguous()
                rects_host = rects.cpu() if rects_host is None else rects_host.to(torch.int32).contiguous()
            ops.image_ingest_resize(src, rects, rects_host, image, masked, flags, flip, norm, PATCH, FILL)
        return dict(image=image, masked_images=masked, patch_flags=flags.view(B, H // PATCH, W // PATCH), flip=flip)


def content_rect(u8_hwc):
    """(y0, x0, h, w) of the reference's content crop (mcloader/fashion_gen.py:416-424) for a decoded uint8 (h, w, 3) image (numpy array or tensor): the
    bounding box of the pixels that are not white after Pillow's `convert('1')`, with the right / bottom edge EXCLUSIVE as the reference writes it
    (`img.crop((w_top, h_top, w_bottom, h_bottom))` with the max index as the far corner: the last content row and column are cut).  Nothing is cropped here: the
    rectangle goes to the device with the whole image (`rects` of DeviceBatchPrep).  Where the reference fails -- a blank image, content on a single row or
    column -- this returns the whole image, respectively a side of 1.  Host helper for loaders, which decode with Pillow anyway: needs PIL."""
    import numpy as np
    from PIL import Image
    arr = np.ascontiguousarray(u8_hwc.numpy() if isinstance(u8_hwc, torch.Tensor) else u8_hwc)
    assert arr.dtype == np.uint8 and arr.ndim == 3 and arr.shape[2] == 3
    ys, xs = (np.array(Image.fromarray(arr).convert("1")) == False).nonzero()       # noqa: E712 (the reference's comparison)
    if ys.size == 0:
        return 0, 0, arr.shape[0], arr.shape[1]
    y0, x0 = int(ys.min()), int(xs.min())
    return y0, x0, max(1, int(ys.max()) - y0), max(1, int(xs.max()) - x0)


class DevicePrefetcher:
    """Iterate `loader` one batch ahead on a side stream.  Every tensor of a sample dict is staged through pinned memory and
    copied asynchronously; with `prep` (a DeviceBatchPrep) the masked image, the masked token ids, the MLM labels and the
    masked-index selection are produced on the device from `image` + `ori_input_ids` instead of being shipped; a uint8 `image` (B,h,w,3), optionally with an
    `image_rects` key (int32 (B,4) = y0, x0, h, w), is resized / flipped / converted there as well and replaced by the fp32 result.  Yields dicts
    of device tensors plus `mlm_positions` / `mlm_count` (host int) when the selection was made here."""

    def __init__(self, loader, device, prep=None):
        self.loader, self.device, self.prep = loader, torch.device(device), prep
        self.stream = torch.cuda.Stream(self.device)
        self._pins = {}

    def __len__(self):
        return len(self.loader)

    def _stage(self, key, t):
        if t.is_cuda:
            return t
        pin = self._pins.get(key)
        if pin is None or pin[0].shape != t.shape or pin[0].dtype != t.dtype:
            pin = self._pins[key] = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for _ in range(2)]      # double-buffered
        buf = pin[self._flip]
        buf.copy_(t)
        return buf.to(self.device, non_blocking=True)

    def _preload(self, it):
        try:
            samples = next(it)
        except StopIteration:
            return None
        self._flip ^= 1
        with torch.cuda.stream(self.stream):
            batch = {k: (self._stage(k, v) if isinstance(v, torch.Tensor) else v) for k, v in samples.items()}
            cnt_pin = None
            if self.prep is not None:
                kw = {}
                if "image_rects" in batch:                     # uint8 slabs: one source rectangle per sample; the loader's own CPU tensor is what gets checked
                    host = samples["image_rects"]
                    kw = dict(rects=batch["image_rects"], rects_host=None if host.is_cuda else host)
                made = self.prep(batch["image"], batch["ori_input_ids"], **kw)
                if "image" in made:                            # uint8 in: the engine sees the fp32 image, as always
                    batch.update(image=made["image"], flip=made["flip"])
                batch.update(masked_images=made["masked_images"], input_ids=made["input_ids"], mlm_labels=made["mlm_labels"],
                             patch_flags=made["patch_flags"])
                idx, cnt = made["mlm_positions_buf"], made["mlm_count_dev"]
            elif "mlm_labels" in batch and "mlm_positions" not in batch:
                lab = batch["mlm_labels"].reshape(-1).contiguous()
                idx = torch.empty(lab.numel(), device=self.device, dtype=torch.int32)
                cnt = torch.zeros(1, device=self.device, dtype=torch.int32)
                ops.masked_select(lab, idx, cnt)
            else:
                idx = cnt = None
            if cnt is not None:
                cnt_pin = self._cnt_pins[self._flip]
                cnt_pin.copy_(cnt, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return batch, idx, cnt_pin, ev

    def __iter__(self):
        self._flip = 0
        self._cnt_pins = [torch.empty(1, dtype=torch.int32).pin_memory() for _ in range(2)]
        it = iter(self.loader)
        nxt = self._preload(it)
        while nxt is not None:
            batch, idx, cnt_pin, ev = nxt
            ev.synchronize()                                   # the side stream finished this batch long ago (one step of lead)
            cur = torch.cuda.current_stream(self.device)
            cur.wait_stream(self.stream)
            for v in batch.values():
                if isinstance(v, torch.Tensor) and v.is_cuda:
                    v.record_stream(cur)
            if idx is not None:
                n = int(cnt_pin[0])
                idx.record_stream(cur)
                batch["mlm_positions"], batch["mlm_count"] = idx[:n], n
            nxt = self._preload(it)                            # next batch starts copying while this one computes
            yield batch
