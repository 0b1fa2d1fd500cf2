# -*- coding: utf-8 -*-
"""
PNG files made on the device: the last step of the reference's dataset inference run
(/root/reference/inference_dataset.py:212-237, 273-307, 372-399, 430 -- every `scannet-*` output is a PNG
written with `cv2.imwrite`).  `InferenceOutputPacker` leaves the dense maps in HBM; here each image of
such a stack becomes one complete PNG file, still in HBM, and only the files cross to the host: label
maps compress to a few percent of their size, and the host deflates nothing.
Kernels: csrc/png.hip (filter 0, fixed-Huffman deflate whose matches are runs of equal pixels, CRC-32
and Adler-32 on the device); rules: include/emsanet_hip.h.

    enc = PngEncoder(ring=2)
    files = enc.to_host(enc.encode(stack))            # list of M memoryviews, each a whole .png
    by_key = {k: enc.to_host(e) for k, e in enc.encode_packed(packer.pack(prediction, batch)).items()}
    write_scannet_output(by_key, filenames, output_path)

Layouts (the stack's dtype and shape name them):
    GRAY8    uint8  (M, H, W)      semantic maps, instance mask planes
    BGR8     uint8  (M, H, W, 3)   panoptic / three-channel ground truth, B, G, R as cv2.imwrite is given
    GRAY16   uint16 (M, H, W)      sem * 1000 + inst ground truth
`encode` launches kernels only -- no host copy, no synchronisation, after the first `ring` calls for a
shape no allocation -- so it can follow `pack` inside a captured graph.  `to_host` is the one call that
synchronises: it reads the offsets table and copies only the bytes the files take.

The other direction -- the training inputs the reference's datasets store as PNG files -- is `PngDecoder`
(kernels: csrc/png_decode.hip, csrc/png_inflate_core.h): any deflate stream, IDAT chunks split anywhere, all
five filter types, for the same three layouts; palette, alpha, 16-bit RGB, depths below 8 and interlaced
files are refused by name from the IHDR.  Chunk CRC-32s are not verified, the Adler-32 is.

    files = PngFiles.from_bytes(list_of_file_bytes)   # one pinned buffer + offsets; all of one layout / size
    dec = PngDecoder(ring=2)                          # order='rgb': what BatchStager / TrainingAugmenter read
    stack = dec.decode(files.to(device))              # kernels only -> uint8 (M,H,W[,3]) / uint16 (M,H,W)
    dec.check()                                       # the one synchronising call: PngDecodeError names the file
    BatchStager(batches_of_PngFiles, device, decoder=dec, augmenter=..., target_generator=...)
"""
import os
import struct

import torch

GRAY8, BGR8, GRAY16 = 0, 1, 2                      # EMSA_PNG_* of include/emsanet_hip.h
LAYOUTS = (GRAY8, BGR8, GRAY16)
MAX_SIDE = 4096                                    # EMSA_PNG_MAX_SIDE; the MAX_SIDE of augment.py
STRIP_ROWS = 4                                     # rows per deflate block / IDAT chunk (csrc/png.hip)
_BPP = {GRAY8: 1, BGR8: 3, GRAY16: 2}
_DTYPE = {GRAY8: torch.uint8, BGR8: torch.uint8, GRAY16: torch.uint16}


def _strip_bound(n, last):
    return (9 * n + 20) // 8 + 4 + (5 if last else 0)


def png_bound(layout, h, w):
    """the most bytes one file of an (h, w) image can take -- emsa_png_bound, restated so that it needs no
    library: per strip of 4 rows 3 header bits, 9 bits per scanline byte (a literal >= 144), the end of
    block, the byte-aligning empty stored block; signature, IHDR, IEND, zlib header, the closing block
    and Adler-32; 12 bytes of chunk framing per strip"""
    if layout not in LAYOUTS:
        raise ValueError(f"png_bound: unknown layout {layout}; GRAY8 (0), BGR8 (1) or GRAY16 (2)")
    h, w = int(h), int(w)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"png_bound: size {h} x {w}; sides of 1 ... {MAX_SIDE}")
    rowlen = 1 + w * _BPP[layout]
    strips = (h + STRIP_ROWS - 1) // STRIP_ROWS
    last_rows = h - (strips - 1) * STRIP_ROWS
    return 51 + 12 * strips + (strips - 1) * _strip_bound(STRIP_ROWS * rowlen, False) + \
        _strip_bound(last_rows * rowlen, True)


def infer_layout(stack):
    """GRAY8 / BGR8 / GRAY16 from a stack's dtype and shape (TypeError / ValueError otherwise)"""
    if not torch.is_tensor(stack):
        raise TypeError("PngEncoder: the stack must be a tensor")
    if stack.dtype == torch.uint8:
        if stack.dim() == 3:
            return GRAY8
        if stack.dim() == 4 and stack.shape[3] == 3:
            return BGR8
        raise ValueError(f"PngEncoder: a uint8 stack is (M, H, W) or (M, H, W, 3), got {tuple(stack.shape)}")
    if stack.dtype in (torch.uint16, torch.int16):
        if stack.dim() == 3:
            return GRAY16
        raise ValueError(f"PngEncoder: a uint16 stack is (M, H, W), got {tuple(stack.shape)}")
    raise TypeError(f"PngEncoder: the stack has dtype {stack.dtype}; uint8 or uint16")


def _check_stack(stack, layout):
    """-> (layout, m, h, w) of a stack that the kernels can read, or the refusal"""
    inferred = infer_layout(stack)
    if layout is None:
        layout = inferred
    elif layout not in LAYOUTS:
        raise ValueError(f"PngEncoder: unknown layout {layout}")
    elif layout != inferred:
        raise ValueError(f"PngEncoder: layout {layout} against a {stack.dtype} stack {tuple(stack.shape)}")
    m, h, w = (int(v) for v in stack.shape[:3])
    if m < 1 or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"PngEncoder: stack {tuple(stack.shape)}: at least one image, sides of 1 ... {MAX_SIDE}")
    if not stack.is_cuda:
        raise NotImplementedError("PngEncoder: the stack is a CPU tensor; the files are encoded on the GPU only")
    return layout, m, h, w


class EncodedStack:
    """what `encode` returns: data uint8 (M * bound,) and offsets int64 (M + 1,) on the device -- file i is
    data[offsets[i]:offsets[i + 1]] -- the number of files and the ring set the buffers belong to"""
    __slots__ = ('data', 'offsets', 'm', 'turn', 'key')

    def __init__(self, data, offsets, m, turn, key=None):
        self.data, self.offsets, self.m, self.turn, self.key = data, offsets, m, turn, key

    def __iter__(self):
        return iter((self.data, self.offsets, self.m, self.turn))


class PngEncoder:
    """see the module docstring.  Device buffers (files, offsets, scratch) are kept per shape and rotate
    over `ring` sets as the packer's do: the result of call k stays intact until call k + ring."""

    def __init__(self, ring=2):
        if int(ring) < 1:
            raise ValueError("PngEncoder: ring must be >= 1")
        self.ring = int(ring)
        self._turn = -1
        self._buf = {}
        self._pinned = {}

    def _buffers(self, key, m, bound, ws_bytes, device):
        b = self._buf.get(key)
        if b is None:
            from . import _lib
            from . import functional as Fn
            if torch.cuda.is_current_stream_capturing():
                raise _lib.EmsaError(f"PngEncoder: no buffers for {key[1:]} yet and the stream is capturing: "
                                     "run encode() `ring` times before capturing")
            b = self._buf[key] = (Fn._empty((m * bound,), device, torch.uint8),
                                  Fn._empty((m + 1,), device, torch.int64),
                                  Fn._empty((ws_bytes,), device, torch.uint8))
        return b

    def _encode(self, stack, layout, turn, tag):
        from . import _lib
        from . import functional as Fn
        layout, m, h, w = _check_stack(stack, layout)
        stack = stack.contiguous()
        L = _lib.lib()
        bound = png_bound(layout, h, w)
        ws_bytes = int(L.emsa_png_ws_bytes(layout, m, h, w))
        if ws_bytes < 0:
            _lib.check(ws_bytes, 'emsa_png_ws_bytes')
        key = (turn, tag, layout, m, h, w, str(stack.device))
        data, offsets, ws = self._buffers(key, m, bound, ws_bytes, stack.device)
        _lib.check(L.emsa_png_encode(stack.data_ptr(), layout, m, h, w, data.data_ptr(), data.numel(),
                                     offsets.data_ptr(), ws.data_ptr(), Fn._stream()), 'emsa_png_encode')
        return EncodedStack(data, offsets, m, turn, key)

    def encode(self, stack, layout=None):
        """every image of `stack` as a PNG file -> EncodedStack; kernels only"""
        _check_stack(stack, layout)                       # a refused call does not advance the ring
        self._turn = (self._turn + 1) % self.ring
        return self._encode(stack, layout, self._turn, None)

    def encode_packed(self, packed):
        """every tensor of a `PackedOutputs` under a `scannet_*` key -> {key: EncodedStack}, the layout by
        dtype; `mapping/*` entries are left alone.  One turn of the ring for the whole dictionary."""
        todo = [(k, v) for k, v in packed.items() if k.startswith('scannet_') and torch.is_tensor(v)]
        for _, v in todo:
            _check_stack(v, None)
        self._turn = (self._turn + 1) % self.ring
        return {k: self._encode(v, None, self._turn, k) for k, v in todo}

    def to_host(self, encoded):
        """the files of one EncodedStack as a list of M memoryviews, each a complete PNG file.
        SYNCHRONISES: the offsets table is read, then only offsets[M] bytes are copied into a pinned
        buffer of the ring set (the views stay valid until the set comes round again, `ring` calls on)."""
        offsets = encoded.offsets.cpu().tolist()              # <- the synchronisation
        total = offsets[encoded.m]
        if not (offsets[0] == 0 and 0 < total <= encoded.data.numel()):
            raise RuntimeError(f"PngEncoder.to_host: offsets table {offsets[0]} ... {total} against a buffer of "
                               f"{encoded.data.numel()} bytes")
        p = self._pinned.get(encoded.key)
        if p is None or p.numel() < total:
            size = 1 << max(12, (total - 1).bit_length())
            p = self._pinned[encoded.key] = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        p[:total].copy_(encoded.data[:total], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        view = memoryview(p.numpy())
        return [view[offsets[i]:offsets[i + 1]] for i in range(encoded.m)]

    def release(self):
        """drop every device and pinned buffer (earlier results become invalid)"""
        self._buf.clear()
        self._pinned.clear()


def write_scannet_output(files_by_key, filenames, output_path, instance=None, instance_files=None):
    """the directory tree of the reference's `scannet-*` formats from device-made files: plain writes.
    files_by_key: {packer key: list of files}, e.g. 'scannet_semantic/pred_path_semantic' ->
    <output_path>/scannet_semantic/pred_path_semantic/<filenames[i]> (/root/reference/inference_dataset.py:
    221, 261, 282, 296, 350).  instance / instance_files: an `InstanceOutputs` and the files of its `masks`
    stack -> <output_path>/scannet_instance/pred_path_panoptic_instance/predicted_masks/<basename>_<rank:03d>.png
    and <basename>.txt with the lines verbatim (:406-442); basename = the file name without extension.
    -> the paths written"""
    written = []
    for key, files in files_by_key.items():
        if not key.startswith('scannet_'):
            raise ValueError(f"write_scannet_output: '{key}' is not a scannet_* key")
        if len(files) != len(filenames):
            raise ValueError(f"write_scannet_output: {len(files)} files under '{key}' for {len(filenames)} names")
        d = os.path.join(output_path, *key.split('/'))
        os.makedirs(d, exist_ok=True)
        for name, f in zip(filenames, files):
            fn = os.path.join(d, name)
            with open(fn, 'wb') as fh:
                fh.write(f)
            written.append(fn)
    if instance is not None:
        start, lines = instance.start, instance.lines
        files = [] if instance_files is None else instance_files
        if len(lines) != len(filenames) or len(files) != start[-1]:
            raise ValueError(f"write_scannet_output: {len(lines)} samples / {len(files)} mask files against "
                             f"{len(filenames)} names / {start[-1]} masks")
        d = os.path.join(output_path, 'scannet_instance', 'pred_path_panoptic_instance')
        os.makedirs(os.path.join(d, 'predicted_masks'), exist_ok=True)
        for i, name in enumerate(filenames):
            base = os.path.splitext(name)[0]
            for r in range(start[i + 1] - start[i]):
                fn = os.path.join(d, 'predicted_masks', f"{base}_{r:03d}.png")
                with open(fn, 'wb') as fh:
                    fh.write(files[start[i] + r])
                written.append(fn)
            fn = os.path.join(d, base + '.txt')
            with open(fn, 'w') as fh:
                fh.writelines(lines[i])
            written.append(fn)
    return written


# ---- decoding ---------------------------------------------------------------------------------------
RGB, BGR = 0, 1                                    # EMSA_PNGD_RGB / EMSA_PNGD_BGR
MAX_FILE_BYTES = 1 << 30
SIGNATURE = b'\x89PNG\r\n\x1a\n'
STATUS_NAMES = ('ok', 'bad signature or chunk structure', 'IHDR differs from the call', 'truncated stream',
                'bad zlib header', 'bad block type', 'stored block length check', 'invalid code lengths',
                'invalid symbol or distance code', 'distance before the start of the output',
                'too many scanline bytes', 'too few scanline bytes', 'illegal filter type', 'Adler-32 mismatch')
_COLOR_NAMES = {3: 'palette', 4: 'grey with alpha', 6: 'RGB with alpha'}


class PngDecodeError(RuntimeError):
    """raised by PngDecoder.check(): .index = the first bad file of the call, .status = its EMSA_PNGD_* code,
    .failures = [(tag, index, status)] of every bad file"""

    def __init__(self, failures):
        self.failures = failures
        self.tag, self.index, self.status = failures[0]
        what = ', '.join(f"file {i}{'' if t is None else f' of {t!r}'}: {STATUS_NAMES[s] if 0 <= s < 14 else s}"
                         for t, i, s in failures[:8])
        super().__init__(f"PngDecoder: {len(failures)} file(s) not decoded -- {what}")


def png_info(file_bytes):
    """(layout, h, w) of one PNG file from its signature and IHDR alone; ValueError names what the decoder
    does not take"""
    head = bytes(file_bytes[:33])
    if len(head) < 33 or head[:8] != SIGNATURE or head[8:16] != b'\x00\x00\x00\rIHDR':
        raise ValueError("png_info: not a PNG file (signature and IHDR chunk expected in the first 33 bytes)")
    w, h, depth, color, comp, filt, lace = struct.unpack('>IIBBBBB', head[16:29])
    if color in _COLOR_NAMES:
        raise ValueError(f"png_info: {_COLOR_NAMES[color]} images (colour type {color}) are not decoded; "
                         "grey 8 / 16 bit and RGB 8 bit are")
    if color not in (0, 2):
        raise ValueError(f"png_info: unknown colour type {color}")
    if depth < 8:
        raise ValueError(f"png_info: bit depth {depth} is below 8")
    if (color, depth) == (2, 16):
        raise ValueError("png_info: 16-bit RGB is not decoded; RGB files must have 8 bits per sample")
    if depth not in (8, 16):
        raise ValueError(f"png_info: bit depth {depth}")
    if lace:
        raise ValueError("png_info: interlaced (Adam7) files are not decoded")
    if comp or filt:
        raise ValueError(f"png_info: compression method {comp} / filter method {filt}; both must be 0")
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"png_info: size {h} x {w}; sides of 1 ... {MAX_SIDE} (EMSA_PNG_MAX_SIDE)")
    return (BGR8 if color == 2 else GRAY16 if depth == 16 else GRAY8), h, w


class PngFiles:
    """M complete PNG files of one layout and size: data uint8 (bytes,), offsets int64 (M + 1,) -- file i is
    data[offsets[i]:offsets[i + 1]] -- on the host (pinned) or on the device; file_bytes = the most bytes
    one file takes (what the decoder sizes its scratch by)"""
    __slots__ = ('data', 'offsets', 'm', 'layout', 'h', 'w', 'file_bytes', 'total')

    def __init__(self, data, offsets, m, layout, h, w, file_bytes, total=None):
        if layout not in LAYOUTS:
            raise ValueError(f"PngFiles: unknown layout {layout}")
        if not (m >= 1 and 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"PngFiles: {m} files of {h} x {w}: at least one, sides of 1 ... {MAX_SIDE}")
        if not 1 <= file_bytes <= MAX_FILE_BYTES:
            raise ValueError(f"PngFiles: files of up to {file_bytes} bytes; 1 ... {MAX_FILE_BYTES}")
        if data.dtype != torch.uint8 or data.dim() != 1 or offsets.dtype != torch.int64 or \
                tuple(offsets.shape) != (m + 1,) or data.device != offsets.device:
            raise ValueError("PngFiles: data is uint8 (bytes,), offsets int64 (M + 1,), on one device")
        self.data, self.offsets, self.m, self.layout, self.h, self.w = data, offsets, int(m), layout, int(h), int(w)
        self.file_bytes = int(file_bytes)
        self.total = data.numel() if total is None else int(total)      # bytes the files take (host knowledge)

    @classmethod
    def from_bytes(cls, files, pin=True):
        """a list of bytes-like objects, each one whole PNG file -> one (pinned) buffer and its offsets.  Reads
        33 bytes of every file; ValueError names the file that is unsupported or differs from file 0"""
        files = list(files)
        if not files:
            raise ValueError("PngFiles.from_bytes: no files")
        infos = []
        for i, f in enumerate(files):
            try:
                infos.append(png_info(f))
            except ValueError as e:
                raise ValueError(f"PngFiles.from_bytes: file {i}: {e}") from None
            if infos[i] != infos[0]:
                raise ValueError(f"PngFiles.from_bytes: file {i} has layout {infos[i][0]}, size {infos[i][1]} x "
                                 f"{infos[i][2]}; file 0 has layout {infos[0][0]}, size {infos[0][1]} x "
                                 f"{infos[0][2]} (one layout and size per call)")
        sizes = [len(f) for f in files]
        if max(sizes) > MAX_FILE_BYTES:
            raise ValueError(f"PngFiles.from_bytes: file {sizes.index(max(sizes))} has {max(sizes)} bytes; at "
                             f"most {MAX_FILE_BYTES}")
        pin = pin and torch.cuda.is_available()
        data = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=pin)
        offsets = torch.zeros(len(files) + 1, dtype=torch.int64, pin_memory=pin)
        offsets[1:] = torch.tensor(sizes, dtype=torch.int64).cumsum(0)
        view = memoryview(data.numpy())
        pos = 0
        for f, n in zip(files, sizes):
            view[pos:pos + n] = f                                   # (a memcpy per file; no per-byte work)
            pos += n
        layout, h, w = infos[0]
        return cls(data, offsets, len(files), layout, h, w, max(sizes))

    @classmethod
    def from_encoded(cls, encoded, layout=None, h=None, w=None):
        """the files of an `EncodedStack` where they lie, on the device: no copy, no synchronisation
        (layout and size come from the stack's key; a hand-built EncodedStack needs them given)"""
        if encoded.key is not None:
            layout, h, w = encoded.key[2], encoded.key[4], encoded.key[5]
        if layout is None or h is None or w is None:
            raise ValueError("PngFiles.from_encoded: this EncodedStack carries no key; pass layout, h, w")
        return cls(encoded.data, encoded.offsets, encoded.m, layout, h, w, png_bound(layout, h, w))

    def to(self, device, non_blocking=True):
        """the same files on `device` (both tensors copied on the current stream)"""
        return PngFiles(self.data.to(device, non_blocking=non_blocking),
                        self.offsets.to(device, non_blocking=non_blocking), self.m, self.layout, self.h, self.w,
                        self.file_bytes, self.total)


def _capacity(n):
    return 1 << max(12, (int(n) - 1).bit_length())


class PngDecoder:
    """see the module docstring.  Device buffers (stack, status, scratch) come from `functional._empty`, are
    kept per (tag, layout, M, H, W, scratch capacity) and rotate over `ring` sets: the result of call k stays
    intact until call k + ring.  The scratch is sized for files of up to the next power of two of
    `files.file_bytes`, so batches of differing file sizes share it.  order: 'rgb' or 'bgr', the channel
    order of three-channel stacks."""

    def __init__(self, ring=2, order='rgb'):
        if int(ring) < 1:
            raise ValueError("PngDecoder: ring must be >= 1")
        if order not in ('rgb', 'bgr'):
            raise ValueError(f"PngDecoder: order {order!r}; 'rgb' or 'bgr'")
        self.ring = int(ring)
        self.order = order
        self._turn = -1
        self._buf = {}
        self._unchecked = {}                       # buffer key -> (tag, status tensor) of its latest call
        self.status = None                         # int32 (M,) on the device: EMSA_PNGD_* of the latest call

    @staticmethod
    def _check_files(files):
        if not isinstance(files, PngFiles):
            raise TypeError("PngDecoder: decode() takes a PngFiles")
        if not files.data.is_cuda:
            raise NotImplementedError("PngDecoder: the files are in host memory; they are decoded on the GPU "
                                      "only -- files.to(device), or hand them to a BatchStager")

    def _decode(self, files, turn, tag):
        from . import _lib
        from . import functional as Fn
        L = _lib.lib()
        layout, m, h, w = files.layout, files.m, files.h, files.w
        cap = _capacity(files.file_bytes)
        ws_bytes = int(L.emsa_png_decode_ws_bytes(layout, m, h, w, cap))
        if ws_bytes < 0:
            _lib.check(ws_bytes, 'emsa_png_decode_ws_bytes')
        dev = files.data.device
        key = (turn, tag, layout, m, h, w, cap, str(dev))
        b = self._buf.get(key)
        if b is None:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.EmsaError(f"PngDecoder: no buffers for {key[1:]} yet and the stream is capturing: "
                                     "run decode() `ring` times before capturing")
            shape = (m, h, w, 3) if layout == BGR8 else (m, h, w)
            b = self._buf[key] = (Fn._empty(shape, dev, _DTYPE[layout]), Fn._empty((m,), dev, torch.int32),
                                  Fn._empty((ws_bytes,), dev, torch.uint8))
        stack, status, ws = b
        data = files.data.contiguous()
        _lib.check(L.emsa_png_decode(data.data_ptr(), files.offsets.data_ptr(), data.numel(), m, layout,
                                     BGR if self.order == 'bgr' else RGB, h, w, stack.data_ptr(),
                                     status.data_ptr(), ws.data_ptr(), ws.numel(), Fn._stream()),
                   'emsa_png_decode')
        self.status = status
        self._unchecked[key] = (tag, status)
        return stack

    def decode(self, files, tag=None):
        """every file of `files` (a PngFiles on the device) as one image of the stack; kernels only.  A file
        that cannot be decoded leaves an all-zero image and a non-zero entry in `status`."""
        self._check_files(files)                          # a refused call does not advance the ring
        self._turn = (self._turn + 1) % self.ring
        return self._decode(files, self._turn, tag)

    def decode_batch(self, files_by_key):
        """{key: PngFiles} -> {key: stack}: one turn of the ring for the whole dictionary"""
        for f in files_by_key.values():
            self._check_files(f)
        self._turn = (self._turn + 1) % self.ring
        return {k: self._decode(f, self._turn, k) for k, f in files_by_key.items()}

    def check(self):
        """SYNCHRONISES: reads the status of every decode call made since the last check (the latest call per
        buffer set); PngDecodeError names the file index and the cause of the first bad file"""
        pending, self._unchecked = self._unchecked, {}
        if not pending:
            return
        tags = [t for t, _ in pending.values()]
        codes = torch.cat([s for _, s in pending.values()]).cpu().tolist()           # <- the synchronisation
        failures, pos = [], 0
        for tag, (_, s) in zip(tags, pending.values()):
            failures += [(tag, i, c) for i, c in enumerate(codes[pos:pos + s.numel()]) if c != 0]
            pos += s.numel()
        if failures:
            raise PngDecodeError(failures)

    def release(self):
        """drop every device buffer (earlier results become invalid)"""
        self._buf.clear()
        self._unchecked.clear()
        self.status = None
