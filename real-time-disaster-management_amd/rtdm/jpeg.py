"""Device JPEG decode: the decode inside cv2.imread (victim_localization/yolov3/utils/
datasets.py:97 load_image, disaster_detection/aider-predict.py:57) on the HIP runtime.

The bit-serial Huffman entropy decode runs on the host (``rtdm_jpeg_entropy_decode``, C++,
into int16 coefficient blocks in pinned memory); the blocks go to the device, where
dequantisation + islow IDCT (one thread per 8x8 block) and fancy upsampling + YCbCr -> RGB
(one thread per pixel) produce the uint8 [H, W, 3] frame in HBM, bit-exact with
libjpeg-turbo's default decompression, i.e. with cv2.imread / Pillow
(tests/test_gpu_jpeg.py).  Baseline and extended sequential 8-bit Huffman JPEGs (SOF0 /
SOF1; 4:4:4, 4:2:2, 4:2:0, grayscale; restart markers): every JPEG in the reference's
datasets.  ``supported(data)`` is False for progressive / arithmetic / 12-bit streams, which
``decode`` refuses with NotImplementedError (there is no silent host fallback).

A folder of files goes through ``BatchDecoder`` / ``decode_batch``: the same decode for n
streams with the Huffman stage on host threads, one host-to-device copy and two kernel
launches per batch (rtdm_jpeg_batch_plan / _entropy_decode_batch / _reconstruct_batch),
bit-identical to ``decode`` per image (tests/test_gpu_jpeg_batch.py).
"""
from __future__ import annotations

import ctypes
import threading
import time

import numpy as np
import torch

from . import _lib as L


def info(data: bytes) -> L.rtdm_jpeg_info:
    """Header geometry (no entropy decode)."""
    buf = np.frombuffer(data, np.uint8)
    inf = L.rtdm_jpeg_info()
    L.check(L.lib().rtdm_jpeg_info_get(buf.ctypes.data, buf.size, ctypes.byref(inf)))
    return inf


def supported(data: bytes) -> bool:
    try:
        return bool(info(data).supported)
    except L.RtdmError:
        return False


def entropy_decode(data: bytes, pin: bool = False):
    """Host stage: (coef int16 [nblocks, 64], qt int16-viewed uint16 [ncomp, 64], info)."""
    buf = np.frombuffer(data, np.uint8)
    inf = info(data)
    if not inf.supported:
        raise NotImplementedError("rtdm.jpeg: only sequential 8-bit Huffman JPEGs (SOF0 / SOF1) decode on the device")
    coef = torch.empty((inf.nblocks, 64), dtype=torch.int16, pin_memory=pin)
    qt = torch.empty((max(1, inf.ncomp), 64), dtype=torch.int16, pin_memory=pin)
    L.check(L.lib().rtdm_jpeg_entropy_decode(buf.ctypes.data, buf.size, coef.data_ptr(), inf.nblocks, qt.data_ptr(),
                                            ctypes.byref(inf)))
    return coef, qt, inf


def decode(data: bytes, device=None, bgr: bool = False, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """JPEG bytes -> uint8 [H, W, 3] on the device (RGB; BGR with bgr=True, as cv2.imread
    returns it).  Asynchronous on the current (or given) stream."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise ValueError("rtdm.jpeg.decode: the decoder runs on the HIP device (no CPU path)")
    coef, qt, inf = entropy_decode(data, pin=True)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        coef_d = coef.to(dev, non_blocking=True)
        qt_d = qt.to(dev, non_blocking=True)
        ws = torch.empty(int(L.lib().rtdm_jpeg_workspace_bytes(ctypes.byref(inf))), dtype=torch.uint8, device=dev)
        if out is None:
            out = torch.empty((inf.height, inf.width, 3), dtype=torch.uint8, device=dev)
        if out.dtype != torch.uint8 or out.shape != (inf.height, inf.width, 3) or not out.is_contiguous():
            raise ValueError(f"rtdm.jpeg.decode: out must be a contiguous uint8 [{inf.height}, {inf.width}, 3] tensor")
        L.check(L.lib().rtdm_jpeg_reconstruct(coef_d.data_ptr(), qt_d.data_ptr(), ctypes.byref(inf), ws.data_ptr(),
                                             ws.numel(), out.data_ptr(), 3 * inf.width, int(bool(bgr)),
                                             L.stream_ptr(s)))
    return out


def imread(path: str, device=None, bgr: bool = True) -> torch.Tensor:
    """cv2.imread(path) for a JPEG file, decoded on the device (BGR by default, as cv2)."""
    with open(path, "rb") as f:
        return decode(f.read(), device=device, bgr=bgr)


# ---- batched ingest: n streams, host threads for the Huffman stage, one copy, two launches ----

_UNSUPPORTED = "only sequential 8-bit Huffman JPEGs (SOF0 / SOF1; 4:4:4, 4:2:2, 4:2:0, gray) decode on the device"


class BatchPlan:
    """rtdm_jpeg_batch_plan's result for a list of streams: infos / status / items (ctypes
    arrays, one entry per image), layout (rtdm_jpeg_batch_layout) and desc (the descriptor blob,
    uint8 numpy)."""

    def __init__(self, datas, out_off=None, out_pitch=None):
        self.datas = [d if isinstance(d, bytes) else bytes(d) for d in datas]
        n = self.n = len(self.datas)
        self.ptrs = (ctypes.c_char_p * n)(*self.datas)  # the bytes objects' own buffers (no copy)
        self.lens = (ctypes.c_int64 * n)(*[len(d) for d in self.datas])
        self.infos = (L.rtdm_jpeg_info * n)()
        self.status = (ctypes.c_int * n)()
        self.items = (L.rtdm_jpeg_batch_item * n)()
        self.layout = L.rtdm_jpeg_batch_layout()
        self.desc = np.empty(L.jpeg_batch_desc_bytes(n), np.uint8)
        off = (ctypes.c_int64 * n)(*out_off) if out_off is not None else None
        pitch = (ctypes.c_int64 * n)(*out_pitch) if out_pitch is not None else None
        L.check(L.lib().rtdm_jpeg_batch_plan(self.ptrs, self.lens, n, off, pitch, self.infos, self.status, self.items,
                                            ctypes.byref(self.layout), self.desc.ctypes.data, self.desc.size))


def plan_batch(datas, out_off=None, out_pitch=None) -> BatchPlan:
    """Headers of every stream -> the batch's shared-buffer layout (no entropy decode)."""
    return BatchPlan(datas, out_off, out_pitch)


def entropy_decode_batch(plan: BatchPlan, staging: torch.Tensor | None = None, threads: int = 0):
    """Host stage of a planned batch into staging (uint8, CPU, >= plan.layout.staging_bytes;
    allocated when None): (staging, messages).  plan.status is updated per image; messages[i]
    is the failure text of image i ('' when it decoded or was refused by the plan)."""
    lay = plan.layout
    if staging is None:
        staging = torch.empty(max(16, lay.staging_bytes), dtype=torch.uint8)
    if staging.dtype != torch.uint8 or staging.device.type != "cpu" or not staging.is_contiguous():
        raise ValueError("rtdm.jpeg.entropy_decode_batch: staging must be a contiguous uint8 CPU tensor")
    if staging.numel() < lay.staging_bytes:
        raise ValueError("rtdm.jpeg.entropy_decode_batch: staging buffer too small")
    ctypes.memmove(staging.data_ptr(), plan.desc.ctypes.data, lay.desc_bytes)
    stride = 160
    msgs = ctypes.create_string_buffer(max(1, plan.n) * stride)
    L.check(L.lib().rtdm_jpeg_entropy_decode_batch(plan.ptrs, plan.lens, plan.n, plan.items, ctypes.byref(lay),
                                                  staging.data_ptr(), staging.numel(), int(threads), plan.status, msgs,
                                                  stride))
    raw = msgs.raw
    return staging, [raw[i * stride:(i + 1) * stride].split(b"\0", 1)[0].decode() for i in range(plan.n)]


def batch_coefficients(plan: BatchPlan, staging: torch.Tensor, i: int):
    """Image i of a decoded batch as entropy_decode returns it: (coef int16 [nblocks, 64],
    qt int16-viewed uint16 [ncomp, 64]) views into staging."""
    lay, it, inf = plan.layout, plan.items[i], plan.infos[i]
    c0 = lay.coef_offset + it.block0 * 128
    q0 = lay.qt_offset + it.qt_slot * 384
    coef = staging[c0:c0 + it.nblocks * 128].view(torch.int16).view(-1, 64)
    qt = staging[q0:q0 + 128 * max(1, inf.ncomp)].view(torch.int16).view(-1, 64)
    return coef, qt


class DecodedBatch(list):
    """BatchDecoder.decode's result: the list of uint8 [H, W, 3] device tensors in input order
    (None for an image refused under strict=False).  ``stacked`` is the same memory as one
    [N, H, W, 3] tensor when every image decoded and all have one size (the input
    classify_frames / letterbox_frames take), else None."""
    stacked = None


def _raise_for(i: int, status: int, msg: str, data: bytes):
    if status == L.RTDM_E_UNSUPPORTED:
        raise NotImplementedError(f"rtdm.jpeg: image {i}: {_UNSUPPORTED}")
    if not msg:
        try:  # the plan carries no text: the single-image parser names the reason
            info(data)
        except L.RtdmError as e:
            msg = str(e)
    raise L.RtdmError(status, f"image {i}: {msg}")


class BatchDecoder:
    """Batched device JPEG decode with reusable buffers: two pinned staging buffers used in
    turn, one device staging buffer and one device plane workspace, each regrown geometrically
    when a batch needs more.  Per call: rtdm_jpeg_batch_plan (headers), the Huffman stage on
    ``threads`` host threads (None: min(n, 16)) straight into pinned memory, ONE host-to-device
    copy of [descriptors | tables | coefficients] and TWO kernel launches, all asynchronous on
    the stream.  Calls may follow each other without a host synchronise: a pinned buffer is
    overwritten only after the event recorded behind its last copy, and the device buffers are
    handed from call to call in stream order (across streams through an event).  Not
    thread-safe: one decoder per thread."""

    def __init__(self, device=None, threads: int | None = None):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise ValueError("rtdm.jpeg.BatchDecoder: the decoder runs on the HIP device (no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.threads = 0 if threads is None else int(threads)
        self._pin = [None, None]
        self._pin_ev = [None, None]
        self._turn = 0
        self._stage = None
        self._ws = None
        self._done = None
        self.profile = False  # True: time the stages of every call (see timings())
        self._prof = None

    @staticmethod
    def _size(old, need: int) -> int:
        return max(int(need), 2 * (old.numel() if old is not None else 0), 1 << 16)

    def _pinned(self, k: int, need: int) -> torch.Tensor:
        if self._pin_ev[k] is not None:  # the copy that last read this buffer
            self._pin_ev[k].synchronize()
            self._pin_ev[k] = None
        if self._pin[k] is None or self._pin[k].numel() < need:
            self._pin[k] = torch.empty(self._size(self._pin[k], need), dtype=torch.uint8, pin_memory=True)
        return self._pin[k]

    def _device_buf(self, name: str, need: int, s) -> torch.Tensor:
        t = getattr(self, name)
        if t is None or t.numel() < need:
            # the old tensor goes back to the caching allocator, which keeps it until the work
            # queued on every stream recorded below has finished
            t = torch.empty(self._size(t, need), dtype=torch.uint8, device=self.device)
            setattr(self, name, t)
        t.record_stream(s)
        return t

    def _placement(self, out, n):
        """out -> (base pointer, addressable bytes, offsets, pitches, expected (h, w) per image)."""
        if isinstance(out, torch.Tensor):
            if (out.dim() != 4 or out.shape[0] != n or out.shape[3] != 3 or out.dtype != torch.uint8
                    or out.device != self.device or out.stride(3) != 1 or out.stride(2) != 3
                    or out.stride(1) < 3 * out.shape[2] or out.stride(0) < 0):
                raise ValueError("rtdm.jpeg.BatchDecoder.decode: out must be a uint8 [N, H, W, 3] device tensor with "
                                 "packed pixels (row and image strides are free)")
            span = out.untyped_storage().nbytes() - out.storage_offset()
            return (out.data_ptr(), span, [i * out.stride(0) for i in range(n)], [out.stride(1)] * n,
                    [tuple(out.shape[1:3])] * n, [out[i] for i in range(n)])
        outs = list(out)
        if len(outs) != n:
            raise ValueError("rtdm.jpeg.BatchDecoder.decode: out must have one tensor per image")
        for t in outs:
            if (not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8
                    or t.device != self.device or t.stride(2) != 1 or t.stride(1) != 3 or t.stride(0) < 3 * t.shape[1]):
                raise ValueError("rtdm.jpeg.BatchDecoder.decode: every out tensor must be a uint8 [H, W, 3] device "
                                 "tensor with packed pixels (the row stride is free)")
        base = min(t.data_ptr() for t in outs)
        offs = [t.data_ptr() - base for t in outs]
        span = max(o + (t.shape[0] - 1) * t.stride(0) + 3 * t.shape[1] for o, t in zip(offs, outs))
        return base, span, offs, [t.stride(0) for t in outs], [tuple(t.shape[:2]) for t in outs], outs

    def decode(self, datas, bgr: bool = False, out=None, strict: bool = True, stream=None) -> DecodedBatch:
        """JPEG byte strings -> DecodedBatch (a list of uint8 [H, W, 3] device tensors, RGB, or
        BGR with bgr=True, plus ``.stacked``).  The tensors are views into one arena tensor
        allocated per call, or into ``out``: a uint8 [N, H, W, 3] tensor (row and image strides
        free, e.g. a slice of a wider canvas) or a sequence of N [H, W, 3] tensors (row stride
        free), whose shapes must match the images.  strict=True raises at the first refused
        image, naming its index (NotImplementedError: unsupported stream; RtdmError: corrupt)
        before anything is queued; strict=False returns None in that slot."""
        datas = list(datas)
        n = len(datas)
        res = DecodedBatch()
        if n == 0:
            return res
        place = self._placement(out, n) if out is not None else None
        plan = BatchPlan(datas, place[2], place[3]) if place else BatchPlan(datas)
        lay = plan.layout
        if strict:
            for i in range(n):
                if plan.status[i] != L.RTDM_OK:
                    _raise_for(i, plan.status[i], "", plan.datas[i])
        if place:
            for i in range(n):
                inf = plan.infos[i]
                if plan.status[i] == L.RTDM_OK and (inf.height, inf.width) != place[4][i]:
                    raise ValueError(f"rtdm.jpeg.BatchDecoder.decode: image {i} is {inf.height} x {inf.width}, "
                                     f"its out tensor {place[4][i][0]} x {place[4][i][1]}")
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        k = self._turn
        self._turn ^= 1
        pin = self._pinned(k, lay.staging_bytes)
        t0 = time.perf_counter()
        _, msgs = entropy_decode_batch(plan, pin, self.threads)
        host_ms = (time.perf_counter() - t0) * 1e3
        if strict:
            for i in range(n):
                if plan.status[i] != L.RTDM_OK:
                    _raise_for(i, plan.status[i], msgs[i], plan.datas[i])
        ok = [plan.status[i] == L.RTDM_OK for i in range(n)]
        with torch.cuda.stream(s):
            if self._done is not None:  # the device buffers' last use, possibly on another stream
                s.wait_event(self._done)
            stage = self._device_buf("_stage", lay.staging_bytes, s)
            ws = self._device_buf("_ws", max(16, lay.workspace_bytes), s)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if self.profile else None
            if ev:
                ev[0].record(s)
            stage[:lay.staging_bytes].copy_(pin[:lay.staging_bytes], non_blocking=True)
            self._pin_ev[k] = ev[1] if ev else torch.cuda.Event()
            self._pin_ev[k].record(s)
            if place:
                base, span, arena = place[0], place[1], None
            else:
                arena = torch.empty(max(16, lay.out_bytes), dtype=torch.uint8, device=self.device)
                base, span = arena.data_ptr(), arena.numel()
            L.check(L.lib().rtdm_jpeg_reconstruct_batch(stage.data_ptr(), ctypes.byref(lay), ws.data_ptr(), ws.numel(),
                                                       base, span, int(bool(bgr)), L.stream_ptr(s)))
            self._done = ev[2] if ev else torch.cuda.Event()
            self._done.record(s)
        if ev:
            self._prof = (host_ms, ev)
        for i in range(n):
            if not ok[i]:
                res.append(None)
            elif place:
                res.append(place[5][i])
            else:
                it, inf = plan.items[i], plan.infos[i]
                res.append(arena[it.out_off:it.out_off + inf.height * inf.width * 3].view(inf.height, inf.width, 3))
        if all(ok):
            if isinstance(out, torch.Tensor):
                res.stacked = out
            elif place is None and lay.uniform:
                inf = plan.infos[0]
                res.stacked = arena[:n * inf.height * inf.width * 3].view(n, inf.height, inf.width, 3)
        return res

    def timings(self) -> dict:
        """Stages of the last decode() made with profile = True: host Huffman ms (wall clock of
        rtdm_jpeg_entropy_decode_batch), copy ms and device ms (hipEvents around the copy and
        around the two launches).  Waits for that call's last event."""
        if self._prof is None:
            raise RuntimeError("rtdm.jpeg.BatchDecoder.timings: no profiled decode() yet (set profile = True)")
        host_ms, ev = self._prof
        ev[2].synchronize()
        return {"host_huffman_ms": host_ms, "copy_ms": ev[0].elapsed_time(ev[1]), "device_ms": ev[1].elapsed_time(ev[2])}


_decoders = threading.local()


def decode_batch(datas, device=None, **kw) -> DecodedBatch:
    """BatchDecoder.decode on a decoder cached per device (and per calling thread)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    cache = _decoders.__dict__.setdefault("by_device", {})
    if dev not in cache:
        cache[dev] = BatchDecoder(dev)
    return cache[dev].decode(datas, **kw)
