"""Functional Python wrappers over the libunit_hip.so C ABI (include/unit_hip.h).

PyTorch is used here only as plumbing: device memory (torch.empty on the ROCm device), the current HIP stream and
dtype bookkeeping. Every arithmetic step is one of the hand-written HIP kernels; there is no CPU / eager fallback --
a missing extension or a CPU tensor raises.
"""
import ctypes
import os
import math

import torch

from ._lib import _DEBUG_SYNC, check, lib

F32, BF16 = 0, 1
SCALE_CLAMP = math.log(1000.0 / 16)  # Box2BoxTransform scale_clamp (detectron2 default)


def dt(dtype):
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {dtype}")


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("unit_amd ops need tensors on the ROCm device (no CPU fallback)")
    if type(t) is X3:
        raise TypeError("a bf16x3 split tensor (ops.X3) was handed to a kernel that reads plain fp32: convert with ops.as_f32 first")
    return ctypes.c_void_p(t.data_ptr())


class X3(torch.Tensor):
    """A bf16x3 "split" activation (csrc/split.hip): logically fp32 [..., C], physically two bf16 planes per row, [...][2][C] --
    hi = bf16(x), lo = bf16(x - hi) -- in the 4 bytes per element of a float32 tensor of the SAME shape. The subclass is the marker:
    it survives slicing / views / empty_like / cat (row-wise operations are all the plan does to activations), the conv wrappers take
    it, every other wrapper refuses it (`_p`) until `as_f32` has merged the planes. Never do arithmetic on it with torch operators."""


def _px(t):
    """device pointer of a split tensor (or None)"""
    if t is None:
        return None
    if type(t) is not X3:
        raise TypeError("expected a bf16x3 split tensor (ops.X3): convert with ops.as_x3 first")
    return ctypes.c_void_p(t.data_ptr())


def x3_split(x, out=None):
    """fp32 [..., C] -> X3 of the same shape (unit_x3_split)"""
    assert type(x) is not X3 and x.dtype == torch.float32 and x.is_contiguous(), "x3_split: contiguous fp32"
    c = x.shape[-1]
    y = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib().unit_x3_split(_p(x), ctypes.c_void_p(y.data_ptr()), x.numel() // c, c, _s()), "x3_split")
    return y.as_subclass(X3)


def x3_merge(x, out=None):
    """X3 -> plain fp32 of the same shape (hi + lo, exact)"""
    assert type(x) is X3 and x.is_contiguous()
    c = x.shape[-1]
    y = out if out is not None else torch.empty(x.shape, dtype=torch.float32, device=x.device).as_subclass(torch.Tensor)
    check(lib().unit_x3_merge(_px(x), _p(y), x.numel() // c, c, _s()), "x3_merge")
    return y


def as_x3(x):
    return x if (x is None or type(x) is X3) else x3_split(x)


def as_f32(x):
    return x3_merge(x) if type(x) is X3 else x


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


_STREAM_OVERRIDE = []          # stack of raw HIP stream handles: `on_stream` below


def raw_stream(device_index=None):
    """the HIP stream the next launch goes to, as an int: the innermost `on_stream` handle, else torch's current stream.
    torch.cuda.current_stream() builds a Stream object through several Python layers (~4 us, ~750 calls per step = a quarter of
    the step's host time); the raw getter is one C call"""
    if _STREAM_OVERRIDE:
        return _STREAM_OVERRIDE[-1]
    if _raw_stream is None:
        return torch.cuda.current_stream().cuda_stream
    return _raw_stream(torch.cuda.current_device() if device_index is None else device_index)


def _s():
    return ctypes.c_void_p(raw_stream())


class on_stream:
    """`with on_stream(side):` -- the C-ABI launches inside go to the torch.cuda.Stream `side` WITHOUT switching torch's current stream
    (torch.cuda.stream() costs ~15 us of Python per enter / exit, and the step forks ~100 weight-gradient launches per step). Only for
    blocks that launch through this module and allocate nothing whose lifetime depends on the stream; while bench.py's event profiler
    is on, it degrades to torch.cuda.stream (the profiler records torch events on the current stream)."""

    def __init__(self, stream):
        self.stream = stream
        self.ctx = None

    def __enter__(self):
        if PROFILER is not None or torch.cuda.is_current_stream_capturing():
            self.ctx = torch.cuda.stream(self.stream)
            self.ctx.__enter__()
        else:
            _STREAM_OVERRIDE.append(self.stream.cuda_stream)
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        else:
            _STREAM_OVERRIDE.pop()
        return False


def streams_on_distinct_queues(device, n, candidates=12, spin_cycles=200000):
    """-> n torch.cuda.Stream objects that sit on n DIFFERENT hardware queues, none of them the queue of the calling thread's current stream.
    The ROCm runtime maps all HIP streams of a process onto GPU_MAX_HW_QUEUES (4) hardware queues in an order that depends on every stream
    created before -- PyTorch's pool, RCCL's process group ... -- and two streams on one queue run strictly one after the other. Which of the
    step's streams share a queue decides ~10 % of its time (head stream on the main stream's queue, as happens once a process group exists:
    18.2 instead of 16.3 ms), so the choice is made by measurement: two single-wave spin kernels (unit_debug_spin) on two
    streams take one spin time on different queues and two on the same. Costs ~10 ms once. Falls back to fewer distinct streams (roles then
    share a stream OBJECT) when the runtime offers fewer queues."""
    import time
    cur = torch.cuda.current_stream(device)
    sink = torch.zeros(4, dtype=torch.int32, device=device)
    cyc = ctypes.c_longlong(int(spin_cycles))

    def spin(st):
        check(lib().unit_debug_spin(cyc, _p(sink), ctypes.c_void_p(st.cuda_stream)), "debug_spin")

    def pair(a, b):
        best = 1e9
        for _ in range(2):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            spin(a)
            spin(b)
            torch.cuda.synchronize(device)
            best = min(best, time.perf_counter() - t0)
        return best

    cands = [torch.cuda.Stream(device) for _ in range(candidates)]
    spin(cur)
    one = pair(cands[0], cands[0]) / 2.0          # two spins on ONE stream: strictly serial
    share = lambda a, b: pair(a, b) > 1.5 * one
    reps = []
    for c in cands:
        if len(reps) == n:
            break
        if share(c, cur) or any(share(c, r) for r in reps):
            continue
        reps.append(c)
    while len(reps) < n:
        # Fewer distinct queues FOUND than roles -- the runtime offers fewer, or the measurement was disturbed (another process on the same
        # GPU: the two-ranks-one-GPU rehearsals). The roles still get stream OBJECTS of their own (round 6): two of them may then share a
        # hardware queue and run in turn, which costs time, not correctness. Until round 5 the roles were aliased onto one object here; with
        # the weight-gradient and the RPN-branch role on ONE stream object the step's capture makes ROCm 7.2's hipStreamEndCapture segfault
        # (deterministic: UNIT_STREAM_MERGE=wr / all in a single process, profiles/r06_exp_capture_crash_root_cause.txt) -- the "1 in 12-24"
        # crash of DESIGN section 8 round 5 item 10 was this fallback firing when the spin probe of a rank was disturbed by the other rank.
        reps.append(torch.cuda.Stream(device))
    return reps


def stream_wait_stream(waiter, signaller_raw=None):
    """everything enqueued on torch.cuda.Stream `waiter` from now on waits for what is on the stream with raw handle `signaller_raw`
    (default: the current launch stream) so far: one C call (unit_stream_wait_stream) instead of Event() + record + wait_event"""
    sig = raw_stream() if signaller_raw is None else signaller_raw
    check(lib().unit_stream_wait_stream(ctypes.c_void_p(waiter.cuda_stream), ctypes.c_void_p(sig)), "unit_stream_wait_stream")


_WS = {}


def _big_tile_default(dtype, m, k, c, kgemm):
    """use the 256x256 LDS-DMA kernel when it pays (measured, tools/microbench.py): bf16, C % 64 == 0, at least half a
    round of 256x256 tiles and a k-extent long enough to amortise the 128 KB-per-tile epilogue"""
    if dtype != torch.bfloat16 or c % 64 != 0 or k < 256 or kgemm < 512:
        return False
    tiles = ((m + 255) // 256) * ((k + 255) // 256)
    return tiles >= 128


def _four_wave_tile(m, k):
    """the 4-wave LDS-DMA tile (csrc/conv_igemm128.hip) of an [m pixels] x [k channels] layer: 128x64 for 64-channel outputs, 128x128 when
    that gives every CU a workgroup, 64x128 below that (tools/mid_sweep.py: res3, 293 tiles, 22.4 vs 26.2 us with 128x128; res4, 150 tiles,
    27.5 vs 32.9 with 64x128)"""
    if k <= 64:
        return 2
    return 0 if ((m + 127) // 128) * ((k + 127) // 128) >= 256 else 1


def mid_tile_dims(mid):
    """(BM pixels, BN channels) of a `mid` tile code: 0..5 = the 4-wave LDS-DMA tiles, 100 + 10 * (BM / 16) + BN / 64 = loader / consumer tiles
    (+ 2000: their two-workgroups-per-CU form; + 8000: weights fetched straight into registers)"""
    if mid >= 8000:
        mid -= 8000
    code = mid - 2000 if mid >= 2000 else mid
    if code >= 100:
        return (code - 100) // 10 * 16, (code % 10) * 64
    return {0: (128, 128), 1: (64, 128), 2: (128, 64), 3: (64, 128), 4: (96, 128), 5: (96, 128)}[code]


def lc_tile_code(m, k, kgemm):
    """tile of the persistent loader / consumer kernel (csrc/conv_igemm_lc.hip) for an [m pixels] x [k channels] x [kgemm] layer:
    100 + 10 * (BM / 16) + BN / 64. A workgroup's time is its tiles x k-steps x the (BM + BN) * 128 bytes a k-step stages (the CU's
    intake is what bounds it) plus an epilogue per tile; the grid is one workgroup per CU. (M = 9 576, 256 channels: 80 x 128 = 240
    tiles, one per CU, measured best of the eight shapes; 1024 channels: 80 x 256.)"""
    best = None
    for fb, fa in ((4, 2), (5, 2), (6, 2), (7, 2), (8, 2), (4, 4), (5, 4), (6, 4)):
        bm, bn = fb * 16, fa * 64
        tiles = ((m + bm - 1) // bm) * ((k + bn - 1) // bn)
        per_wg = (tiles + 255) // 256
        cost = per_wg * ((kgemm // 64) * (bm + bn) + 0.5 * bm * bn / 64.0)
        if best is None or cost < best[0]:
            best = (cost, 100 + 10 * fb + fa)
    return best[1]


def _mid_tile_default(dtype, m, k, c, kgemm, allow_lc=True):
    """allow_lc=False: the caller's output cannot be written by the loader / consumer kernel (fp32 output, rows not a multiple of 16 bytes):
    choose among the 4-wave tiles only.
    -1: use the register-staged conv_igemm.hip kernel; 0..5: LDS-DMA 4-wave kernel with that tile (csrc/conv_igemm128.hip);
    >= 100: persistent loader / consumer workgroups (csrc/conv_igemm_lc.hip, `lc_tile_code`) -- the layers with a long contraction
    and few output tiles (res4 and the res3 -> res4 transition on four 600x1000 images: 1x1 1024 -> 256 15.0 -> 11.9 us, 3x3 256 -> 256
    26.8 -> 18.9 us, tools/lc_sweep.py); short contractions (K = 256 -> 1024: four k-steps per tile) and the large res2 / res3 maps stay
    on the 4-wave tiles, which measured equal or better there.
    Measured on the backbone shapes (tools/microbench.py): 128x64 for 64-channel outputs, 128x128 when that tiling still
    gives every CU a workgroup or two, 64x128 below that.
    Forms that measured no gain inside the step and are reachable by explicit tile code only: two loader / consumer workgroups per CU
    (+ 2000), weights fetched straight into registers (+ 8000), 96-row tiles (4 / 5) -- profiles/r03_exp_loader_consumer.txt,
    profiles/r06_exp_weights_direct.txt, profiles/r02_exp_mid_sweep_96_row_tiles.txt."""
    if dtype != torch.bfloat16 or c % 64 != 0 or k < 64:
        return -1
    if k <= 64:
        return 2
    tiles = ((m + 127) // 128) * ((k + 127) // 128)
    if allow_lc and kgemm >= 512 and tiles <= 640 and k % 8 == 0:
        return lc_tile_code(m, k, kgemm)
    return _four_wave_tile(m, k)


MID_TILE_POLICY = _mid_tile_default
BIG_TILE_POLICY = _big_tile_default


def select_conv_kernel(dtype, m, k, c, kgemm, out_dtype, ldy, pair=False):
    """the production kernel of a conv layer with m output pixels, k filters, c input channels and a contraction of kgemm = r * s * c:
    (big, mid) -- big: the 256x256 kernel (unit_conv2d_fwd_big, variant 0); else mid >= 0: that tile of unit_conv2d_fwd_mid; else the
    register-staged unit_conv2d_fwd. pair: for unit_conv2d_fwd_pair (m = the pixels of both problems), whose big kernel writes rows of
    16-byte vectors and whose mid kernel has no instantiation of tile 3 and of the two-workgroups-per-CU loader / consumer forms."""
    if BIG_TILE_POLICY(dtype, m, k, c, kgemm) and not (pair and ldy % 8):
        return True, -1
    lc_ok = out_dtype == torch.bfloat16 and ldy % 8 == 0        # the loader / consumer kernel writes bf16 rows of 16-byte vectors
    mid = MID_TILE_POLICY(dtype, m, k, c, kgemm, allow_lc=lc_ok)
    if (mid >= 100 and not lc_ok) or (pair and (2000 <= mid < 8000 or mid == 3)):
        mid = _four_wave_tile(m, k)
    return False, mid


# explicit `tile_cfg` codes of conv2d (tests, tools/, profiles/ name them): code -> ("big", variant of unit_conv2d_fwd_big) or
# ("mid", tile of unit_conv2d_fwd_mid). A code >= 100 is a loader / consumer tile code and goes to unit_conv2d_fwd_mid as it is;
# any other code is the tile_cfg of unit_conv2d_fwd.
TILE_CFG = {
    5: ("big", 0),       # the production kernel (= 8)
    6: ("big", 1),       # two-stage loop, ping-pong wave groups
    7: ("mid", 0),       # 4-wave 128x128
    8: ("mid", 1),       # 4-wave 64 pixels x 128 channels
    9: ("mid", 2),       # 4-wave 128 x 64
    10: ("mid", 3),      # 4-wave 128x128 with in-workgroup split-K
    11: ("big", 2),      # two-stage loop, four 32-k stages
    12: ("big", 3),      # two-stage loop, 224-row tiles
    13: ("big", 4),      # two-stage loop, one barrier per k-tile
    14: ("big", 6),      # shared input super-tile (3x3 s1 p1 on 7x7 maps)
    15: ("big", 7),      # four phases per k-tile
    16: ("big", 8),      # ... with the fragment reads inside the MFMA sections
    17: ("big", 9),      # 8 on 224-row tiles
    18: ("big", 10),     # 8 on 224 or 256 rows, whichever needs fewer rounds x rows
    19: ("mid", 4),      # 4-wave 96 x 128, three LDS stages
    20: ("mid", 5),      # 4-wave 96 x 128, two LDS stages
    21: ("big", 11),     # the schedule of 8 on v_mfma_f32_32x32x16_bf16
    22: ("big", 12),     # 8 without the position-class tiles
    23: ("big/first-loop", 13),     # 8 with the kernel's first main loop (conv_igemm256p8.hip SCHED 0): the A/B partner of the production loop
}

# side HIP stream for the weight-gradient kernels (set by the model when stream overlap is enabled; None = inline)
WGRAD_STREAM = None
# True while a SECOND backbone backward of the same step runs (ragged supervised / weak batches): weight gradients accumulate
WGRAD_ACCUMULATE = False
# True inside the module-level training backward (modeling/train_modules.py): conv weight gradients go straight into `.grad`, not through the
# fused step's multi-tensor plan (slabs + bucket reductions)
WGRAD_DIRECT = False

# bench.py sets this to a dict to time every conv_igemm launch with HIP events on the launch stream (roofline evidence)
PROFILER = None


class _timed:
    """`with _timed("name", flops, bytes):` -- when bench.py has set PROFILER, brackets the launches inside with a HIP-event pair on
    the launch stream and files (e0, e1, flops, algorithmic bytes, ref_bytes | None) under `name`; free otherwise. Figures that cost
    something to work out are set inside the block (`as t: ... if t.prof is not None: t.flops, t.nbytes = ...`)"""

    __slots__ = ("name", "flops", "nbytes", "ref_bytes", "prof", "e0")          # (every conv launch of an eager step passes through here)

    def __init__(self, name, flops=0.0, nbytes=0.0, ref_bytes=None):
        self.name, self.flops, self.nbytes, self.ref_bytes = name, flops, nbytes, ref_bytes

    def __enter__(self):
        self.prof = PROFILER
        if self.prof is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.prof is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.prof.setdefault(self.name, []).append((self.e0, e1, self.flops, self.nbytes, self.ref_bytes))
        return False


_WS_RETIRED = []
_GRAPHS_ALIVE = [False]          # set by engine.GraphedStep at its first capture: from then on an outgrown buffer's address may be baked into a graph


def retain_retired_buffers():
    """engine.GraphedStep, before its first capture: outgrown workspaces / weight-gradient slabs are kept alive from now on (a captured
    hipGraph replays into the addresses it recorded). Without a graph they are returned to the allocator."""
    _GRAPHS_ALIVE[0] = True


WS_GROWTHS = [0]          # scratch / slab buffers replaced by bigger ones so far (bench.py --shapes voc reports the count per run)


def _retire(buf):
    """an outgrown scratch buffer: kept for ever only while a captured graph may replay into it; otherwise handed back to the caching
    allocator -- after the work already queued on the LAUNCH stream (which need not be torch's current stream: `on_stream`), hence the
    record_stream. With multi-scale inputs (ResizeShortestEdge 480-800) the per-conv slabs regrow many times; keeping every old one pinned
    tens of MB each for the life of the process."""
    WS_GROWTHS[0] += 1
    if _GRAPHS_ALIVE[0]:
        _WS_RETIRED.append(buf)
    elif buf.is_cuda:
        buf.record_stream(torch.cuda.ExternalStream(raw_stream(buf.device.index), device=buf.device))


def _grown(nbytes, old):
    """new capacity for a buffer that must hold nbytes: geometric (x1.25 over the old size at least) so that a slowly rising maximum does
    not reallocate at every step"""
    have = old.numel() if old is not None else 0
    return max(int(nbytes), have + have // 4)


def workspace(nbytes, device, slot=0):
    """scratch buffer for the kernels that need one; one buffer per (slot, HIP stream): the step runs the RPN-loss branch,
    the proposal chain and the weight gradients on different streams at the same time, and scratch must never be shared
    between kernels that are not ordered by a stream"""
    key = (device, slot, raw_stream(device.index) if device.type == "cuda" else 0)
    w = _WS.get(key)
    if w is None or w.numel() < nbytes:
        if w is not None:
            _retire(w)      # a captured hipGraph (engine.GraphedStep) may have this address baked into its launches: see _retire
        w = torch.empty(max(_grown(nbytes, w), 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = w
    return w


# ------------------------------------------------------------------------------------------------ a1
def preprocess_images(images, pixel_mean, pixel_std, dtype=torch.bfloat16, cpad=8, normalize_images=False, out=None):
    """images: list of CHW fp32 device tensors (0..255). -> ([N,Hmax,Wmax,cpad] NHWC, [(h,w)...])  rcnn.py:257-266"""
    sizes = [(int(x.shape[-2]), int(x.shape[-1])) for x in images]
    hm, wm = max(s[0] for s in sizes), max(s[1] for s in sizes)
    n = len(images)
    if out is None:
        out = torch.empty((n, hm, wm, cpad), dtype=dtype, device=images[0].device)
    mean = (ctypes.c_float * 3)(*[float(v) for v in pixel_mean])
    std = (ctypes.c_float * 3)(*[float(v) for v in pixel_std])
    for i, x in enumerate(images):
        x = x.contiguous()
        if x.dtype != torch.float32:
            raise TypeError("preprocess_images expects fp32 CHW images")
        check(lib().unit_preprocess_image(_p(x), x.shape[0], sizes[i][0], sizes[i][1], mean, std,
                                          255.0 if normalize_images else 1.0, _p(out[i]), dt(dtype), hm, wm, cpad, _s()),
              "unit_preprocess_image")
    return out, sizes


def image_chw_to_u8(img):
    """CHW fp32 (values in [0, 256), truncated toward zero) or CHW uint8 device image -> uint8 HWC: `image.permute(1, 2, 0).numpy().astype(np.uint8)`
    of the reference's TTA (meta_arch/rcnn.py:216-218) without a stock operator"""
    if img.dim() != 3 or img.dtype not in (torch.float32, torch.uint8):
        raise TypeError("image_chw_to_u8 expects a CHW fp32 or uint8 image")
    img = img.contiguous()
    c, h, w = img.shape
    out = torch.empty((h, w, c), dtype=torch.uint8, device=img.device)
    check(lib().unit_image_chw_to_u8(_p(img), int(img.dtype == torch.uint8), c, h, w, _p(out), _s()), "image_chw_to_u8")
    return out


def tta_view_table(h, w, views):
    """views [(new_h, new_w, flip)...] of an (h, w) image -> host float32 [V, 4] = (sx, sy, flip, W) for tta_boxes: the quotients in double,
    rounded once, as numpy multiplies a float32 array by a python float"""
    return torch.tensor([[new_w * 1.0 / w, new_h * 1.0 / h, float(bool(flip)), float(new_w)] for new_h, new_w, flip in views],
                        dtype=torch.float64).to(torch.float32).reshape(-1, 4)


def tta_boxes(props, count, views, pcap=None):
    """props [P,4] fp32, count device int32 [1] or None, views device fp32 [V,4] (tta_view_table) -> [V,Pcap,4]: every view's proposals
    by Detectron2's float32 apply_box + clip(min=0) rule (unit_tta_boxes); rows >= count are zeros"""
    p = props.shape[0]
    pcap = p if pcap is None else int(pcap)
    v = views.shape[0]
    out = torch.empty((v, pcap, 4), dtype=torch.float32, device=views.device)
    check(lib().unit_tta_boxes(_p(props) if p else None, _p(count), p, pcap, _p(views), v, _p(out), _s()), "tta_boxes")
    return out


def nchw_to_nhwc(x, dtype=torch.bfloat16, cpad=None):
    n, c, h, w = x.shape
    cp = cpad or c
    y = torch.empty((n, h, w, cp), dtype=dtype, device=x.device)
    check(lib().unit_nchw_to_nhwc(_p(x.contiguous().float()), _p(y), dt(dtype), n, c, h, w, cp, _s()), "nchw_to_nhwc")
    return y


def nhwc_to_nchw(x, c=None):
    n, h, w, cp = x.shape
    c = c or cp
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    check(lib().unit_nhwc_to_nchw(_p(x.contiguous()), dt(x.dtype), _p(y), n, c, h, w, cp, _s()), "nhwc_to_nchw")
    return y


def zeros(shape, dtype, device):
    """torch.zeros by the library's own fill kernel (unit_fill_zero): the step launches no stock fill"""
    t = torch.empty(shape, dtype=dtype, device=device)
    check(lib().unit_fill_zero(_p(t), t.numel() * t.element_size(), _s()), "fill_zero")
    return t


def zero_(t):
    """t.zero_() for a contiguous tensor by the library's own fill kernel"""
    assert t.is_contiguous()
    check(lib().unit_fill_zero(_p(t), t.numel() * t.element_size(), _s()), "fill_zero")
    return t


def cast(x, dtype):
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(lib().unit_cast(_p(x.contiguous()), dt(x.dtype), _p(y), dt(dtype), x.numel(), _s()), "cast")
    return y


def shard_sum(parts, out):
    """out[i] = parts[0][i] + parts[1][i] + ... in that order, fp32 (parts: [nparts, n] fp32 / bf16, contiguous; out: fp32 [n]);
    the owner-side sum of the "direct" gradient exchange (parallel.GradBuckets(mode="direct"))"""
    assert parts.dim() == 2 and parts.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == parts.shape[1]
    check(lib().unit_shard_sum(_p(parts), dt(parts.dtype), parts.shape[0], parts.shape[1], _p(out), _s()), "shard_sum")
    return out


def add_cast(a32, b, dtype, mask_ref=None, out=None):
    """y = cast((a32 [+ b]) [* (mask_ref > 0)])"""
    y = out if out is not None else torch.empty(a32.shape, dtype=dtype, device=a32.device)
    check(lib().unit_add_cast(_p(a32), _p(b), _p(mask_ref), _p(y), dt(dtype), a32.numel(), _s()), "add_cast")
    return y


# ------------------------------------------------------------------------------------------------ conv
def conv_out_size(h, w, r, s, stride, pad):
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1


_POLICY_CACHE = {}


def _conv_geometry(x, r, s, stride, pad, scatter):
    """(n, h, w, oh, ow, oy_mul, ohf, owf) of a conv over x [N,H,W,C]. scatter = (oy_mul, OHf, OWf): output pixel (n,oh,ow) lands at
    (n, oh*oy_mul, ow*oy_mul) of an [N,OHf,OWf,.] tensor; None: the plain [N,OH,OW,.] output"""
    n, h, wd = x.shape[:3]
    oh, ow = conv_out_size(h, wd, r, s, stride, pad)
    oy_mul, ohf, owf = (1, oh, ow) if scatter is None else scatter
    return n, h, wd, oh, ow, oy_mul, ohf, owf


def _conv_out(geo, ldy, dtype, device, scattered, x3=False):
    """a conv's output [N,OHf,OWf,ldy] for a geometry of _conv_geometry: zeroed when the launch scatters into it; x3: an ops.X3"""
    shape = (geo[0], geo[6], geo[7], ldy)
    y = zeros(shape, dtype, device) if scattered else torch.empty(shape, dtype=dtype, device=device)
    return y.as_subclass(X3) if x3 else y


def _conv_timed_name(big, dma):
    """the `_timed` name of a forward conv launch: the 256x256 kernels, the LDS-DMA (4-wave / loader-consumer) kernels, the register-staged one"""
    return "conv_igemm256" if big else ("conv_igemm_dma" if dma else "conv_igemm")


def conv2d(x, w, k, r, s, stride=1, pad=0, bias=None, residual=None, mask_ref=None, relu=False, out_dtype=None,
           out=None, ldy=None, scatter=None, tile_cfg=0):
    """x [N,H,W,C] NHWC ; w [k][r][s][C] (same dtype). Returns y [N,OH,OW,ldy] (or writes the strided scatter target).
    scatter = (oy_mul, OHf, OWf): output pixel (n,oh,ow) lands at (n, oh*oy_mul, ow*oy_mul) of `out` [N,OHf,OWf,ldy].
    x an ops.X3 (bf16x3 split tensor, w prepared by weight_prep_x3): conv2d_x3."""
    if type(x) is X3:
        assert out_dtype is None and ldy is None
        return conv2d_x3(x, w, k, r, s, stride, pad, bias=bias, residual=residual, mask_ref=mask_ref, relu=relu, out=out, scatter=scatter,
                         tile=None if tile_cfg == 0 else tile_cfg)
    c = x.shape[3]
    geo = n, h, wd, oh, ow, oy_mul, ohf, owf = _conv_geometry(x, r, s, stride, pad, scatter)
    out_dtype = out_dtype or x.dtype
    ldy = ldy or ((k + 3) // 4 * 4)
    if out is None:
        out = _conv_out(geo, ldy, out_dtype, x.device, scatter is not None)
    big, mid, variant = False, -1, 0
    if tile_cfg == 0:          # the two policy functions cost ~5 us per call (the loader / consumer tile search): cached per shape
        pkey = (x.dtype, n * oh * ow, k, c, r * s * c, out_dtype, ldy % 8, BIG_TILE_POLICY, MID_TILE_POLICY)
        pol = _POLICY_CACHE.get(pkey)
        if pol is None:
            pol = _POLICY_CACHE[pkey] = select_conv_kernel(x.dtype, n * oh * ow, k, c, r * s * c, out_dtype, ldy)
        big, mid = pol
    elif tile_cfg >= 100:
        mid = tile_cfg
    elif tile_cfg in TILE_CFG:
        kind, code = TILE_CFG[tile_cfg]
        if kind.startswith("big"):
            big, variant = True, code
        else:
            mid = code
    with _timed(_conv_timed_name(big and mid < 0, mid >= 0)) as t:
        if mid >= 0:
            check(lib().unit_conv2d_fwd_mid(_p(x), _p(w), _p(out), _p(bias), _p(residual), _p(mask_ref), dt(out_dtype),
                                            n, h, wd, c, k, r, s, stride, pad, oh, ow, ldy, oy_mul, ohf, owf, int(relu), mid, _s()),
                  "unit_conv2d_fwd_mid")
        elif big:
            check(lib().unit_conv2d_fwd_big(_p(x), _p(w), _p(out), _p(bias), _p(residual), _p(mask_ref), dt(out_dtype),
                                            n, h, wd, c, k, r, s, stride, pad, oh, ow, ldy, oy_mul, ohf, owf, int(relu),
                                            variant, _s()),
                  "unit_conv2d_fwd_big")
        else:
            check(lib().unit_conv2d_fwd(_p(x), _p(w), _p(out), _p(bias), _p(residual), _p(mask_ref), dt(x.dtype), dt(out_dtype),
                                        n, h, wd, c, k, r, s, stride, pad, oh, ow, ldy, oy_mul, ohf, owf, int(relu), tile_cfg, _s()),
                  "unit_conv2d_fwd")
        if t.prof is not None:
            es = out.element_size()
            t.flops = 2.0 * n * oh * ow * k * r * s * c
            t.nbytes = (x.numel() + w.numel()) * x.element_size() + n * oh * ow * ldy * es * (1 + (residual is not None) + (mask_ref is not None))
            if mid >= 0:          # operand bytes the busiest CU stages into LDS (feed-bound ceiling of the backbone layers, bench.py backbone_ceiling)
                bm, bn = mid_tile_dims(mid)
                tiles = ((n * oh * ow + bm - 1) // bm) * ((k + bn - 1) // bn)
                t.ref_bytes = ((tiles + 255) // 256) * (r * s * c // 64) * (bm + bn) * 128.0
    return out


FUSE_EPILOGUE = os.environ.get("UNIT_FUSE_EPILOGUE", "1") != "0"          # Res5 heads: average pool + ReLU bit mask inside the last conv's epilogue (conv2d_ex); False = separate kernels


def conv_ex_supported(dtype, c, ldy):
    return dtype == torch.bfloat16 and c % 64 == 0 and ldy % 64 == 0


class ReluBits:
    """(map > 0) of an [R, bins, C] activation as one bit per element in the conv epilogue's order (include/unit_hip.h,
    unit_conv2d_fwd_big_ex); `self[a:b]` = the RoIs a..b of it (same storage, RoI offset)."""

    def __init__(self, data, r, bins, c, roi0=0):
        self.data, self.r, self.bins, self.c, self.roi0 = data, r, bins, c, roi0

    def __getitem__(self, sl):
        start, stop, step = sl.indices(self.r)
        assert step == 1
        return ReluBits(self.data, stop - start, self.bins, self.c, self.roi0 + start)

    def aligned(self):
        """the same RoIs as a ReluBits with RoI offset 0 (what a conv epilogue can read as mask_bits), or None when the offset is not
        a whole number of 128-row wave tiles"""
        m0 = self.roi0 * self.bins
        if m0 % 128:
            return None
        return self if m0 == 0 else ReluBits(self.data[(m0 // 128) * (self.c // 64) * 1024:], self.r, self.bins, self.c, 0)

    def unpack(self):
        """-> bool [r, bins, c] (tests)"""
        dev = self.data.device
        m = torch.arange(self.roi0 * self.bins, (self.roi0 + self.r) * self.bins, device=dev).view(-1, 1)
        n = torch.arange(self.c, device=dev).view(1, -1)
        word = ((m >> 7) * (self.c >> 6) + (n >> 6)) * 64 + ((m & 7) * 8 + ((n & 63) >> 3))
        byte = self.data[word * 16 + ((m & 127) >> 3)]
        return ((byte.int() >> (n & 7)) & 1).bool().view(self.r, self.bins, self.c)


def conv2d_ex(x, w, k, r, s, pad=0, bias=None, residual=None, relu=False, mask_bits=None, want_bits=False, pool_rows=0, want_y=True, x2=None, variant=0,
              pooled_out=None):
    """stride-1 bf16 conv on the 256x256 kernel with the extended epilogue (unit_conv2d_fwd_big_ex): returns (y | None, ReluBits |
    None, pooled [N, k] | None). pool_rows: must be OH*OW -- global average pool of each image (= RoI) fused; want_y=False then
    skips writing the map. mask_bits: ReluBits of an [N, OH*OW, k] map (RoI offset 0). x2 [N,H,W,C2]: second input of a 1x1 conv over
    the channel concatenation [x | x2] with w = [k][1][1][C + C2] (C2 a multiple of C)."""
    n, h, wd, c = x.shape
    c2 = 0
    if x2 is not None:
        c2 = x2.shape[3]
        assert r == 1 and s == 1 and pad == 0 and x2.shape[:3] == x.shape[:3] and c2 % c == 0 and x2.dtype == x.dtype and w.shape[-1] == c + c2
    oh, ow = conv_out_size(h, wd, r, s, 1, pad)
    ldy = k
    assert conv_ex_supported(x.dtype, c, ldy), "conv2d_ex: bf16, C % 64 == 0, K % 8 == 0"
    m = n * oh * ow
    y = torch.empty((n, oh, ow, ldy), dtype=x.dtype, device=x.device) if want_y else None
    bits = None
    if want_bits:
        bits = ReluBits(torch.empty(lib().unit_relu_bits_bytes(m, ldy), dtype=torch.uint8, device=x.device), n, oh * ow, k)
    if mask_bits is not None:
        assert mask_bits.roi0 == 0 and mask_bits.r * mask_bits.bins == m and mask_bits.c == k
    part = None
    if pool_rows:
        assert pool_rows == oh * ow
        part = torch.empty(lib().unit_conv_pool_partial_floats(m, ldy), dtype=torch.float32, device=x.device)
    with _timed("conv_igemm256", 2.0 * m * k * r * s * (c + c2)) as t:
        check(lib().unit_conv2d_fwd_big_ex(_p(x), _p(w), _p(y), _p(bias), _p(residual), _p(mask_bits.data if mask_bits is not None else None),
                                           _p(bits.data if bits is not None else None), _p(part), pool_rows,
                                           n, h, wd, c, k, r, s, pad, ldy, int(relu), _p(x2), c2, int(variant), _s()), "unit_conv2d_fwd_big_ex")
        if t.prof is not None:
            t.nbytes = (x.numel() + w.numel() + (x2.numel() if x2 is not None else 0)) * 2 + m * ldy * 2 * (int(want_y) + (residual is not None)) \
                + (m * ldy // 8) * (int(want_bits) + (mask_bits is not None))
    pooled = None
    if pool_rows:
        pooled = pooled_out if pooled_out is not None else torch.empty((n, k), dtype=x.dtype, device=x.device)
        assert pooled.shape == (n, k) and pooled.is_contiguous() and pooled.dtype == x.dtype
        check(lib().unit_pool_finish(_p(part), n, pool_rows, ldy, k, _p(pooled), k, dt(x.dtype), _s()), "unit_pool_finish")
    return y, bits, pooled


def avgpool_bwd_bits(dfeat, bits, ph, pw):
    """dfeat [R,C] bf16, bits: ReluBits of R RoIs -> g [R,PH,PW,C] = bit ? dfeat / (PH*PW) : 0"""
    assert bits.bins == ph * pw and bits.r == dfeat.shape[0] and bits.c == dfeat.shape[1]
    g = torch.empty((bits.r, ph, pw, bits.c), dtype=dfeat.dtype, device=dfeat.device)
    check(lib().unit_avgpool_bwd_bits(_p(dfeat), _p(bits.data), bits.r, bits.roi0, bits.bins, bits.c, _p(g), _s()), "avgpool_bwd_bits")
    return g


def _fit_slab(slab, nbytes, device):
    """the buffer a launch leaves nbytes of split-M slabs in: `slab` when it is large enough, else a new, larger one (the outgrown one
    is retired as workspace() retires its buffers: a captured step may replay into it)"""
    if slab is None or slab.numel() < nbytes:
        if slab is not None:
            _retire(slab)
        slab = torch.empty(_grown(nbytes, slab), dtype=torch.uint8, device=device)
    return slab


def _wgrad_parts(x, dy, k, r, s, stride=1, pad=0):
    """the problems of ONE layer's weight gradient, one per part: (x, dy, (n, h, w, c, oh, ow), plane passes, dtype code of the kernels).
    x / dy: plain tensors, X3 split tensors (X3_WGRAD_PASSES passes of the bf16 kernels over their planes) or ops.Parts of either."""
    for xp, dp in (zip(x, dy) if isinstance(x, Parts) else ((x, dy),)):
        n, h, wd, c = xp.shape
        oh, ow = conv_out_size(h, wd, r, s, stride, pad)
        if type(xp) is X3:
            yield xp, dp, (n, h, wd, c, oh, ow), X3_WGRAD_PASSES, BF16
        else:
            yield xp, dp, (n, h, wd, c, oh, ow), 1, dt(xp.dtype)


def _wgrad_launch(part, k, r, s, stride, pad, ldy, out, scale, accumulate, variant, ws):
    """one part (of _wgrad_parts) through unit_conv2d_wgrad / unit_conv2d_wgrad_x3: dw = `out` reduced from the slabs in `ws` with scale[k]
    folded, or, out None, the slabs left there; with its profiler entry"""
    x, dy, (n, h, wd, c, oh, ow), passes, code = part
    with _timed("conv_wgrad", passes * 2.0 * n * oh * ow * k * r * s * c, (x.numel() + n * oh * ow * ldy) * x.element_size() + 4 * k * r * s * c):
        if type(x) is X3:
            assert type(dy) is X3 and x.is_contiguous() and dy.is_contiguous() and ldy == k
            check(lib().unit_conv2d_wgrad_x3(_px(x), _px(dy), _p(out), _p(scale), n, h, wd, c, k, r, s, stride, pad, oh, ow, k, int(accumulate),
                                             _x3v(variant), _p(ws), ws.numel(), _s()), "unit_conv2d_wgrad_x3" if out is not None else "unit_conv2d_wgrad_x3(partial)")
        else:
            check(lib().unit_conv2d_wgrad(_p(x), _p(dy), _p(out), _p(scale), code, n, h, wd, c, k, r, s, stride, pad, oh, ow, ldy, int(accumulate),
                                          int(variant), _p(ws), ws.numel(), _s()), "unit_conv2d_wgrad" if out is not None else "unit_conv2d_wgrad(partial)")


def conv2d_wgrad(x, dy, k, r, s, stride=1, pad=0, scale=None, out=None, accumulate=False, ldy=None, variant=0):
    """x [N,H,W,C], dy [N,OH,OW,ldy] -> dw fp32 [k,r,s,C] (scale[k] folded). x, dy ops.X3 (bf16x3 split tensors, ldy = k): the bf16x3
    weight gradient."""
    assert ldy is None or type(x) is not X3
    part, = _wgrad_parts(x, dy, k, r, s, stride, pad)
    n, _, _, c, oh, ow = part[2]
    if out is None:
        out = torch.empty((k, r, s, c), dtype=torch.float32, device=x.device)
    nbytes = part[3] * lib().unit_conv2d_wgrad_workspace_bytes(part[4], n, oh, ow, k, r, s, c)
    ws = workspace(nbytes, x.device, slot=2)   # own slot: these launches may run on a side stream next to sort/NMS (slot 0)
    _wgrad_launch(part, k, r, s, stride, pad, ldy or dy.shape[-1], out, scale, accumulate, variant, ws)
    return out


def conv2d_wgrad_partial(x, dy, k, r, s, stride, pad, slab=None, variant=0):
    """split-M partial slabs only (no reduction): returns (slab uint8 tensor, n_splits); slab i = floats [i*k*r*s*C, ...).
    x / dy ops.X3: passes x splits slabs; ops.Parts: the parts' slabs follow each other (n_splits = all of them)."""
    parts = list(_wgrad_parts(x, dy, k, r, s, stride, pad))
    c = parts[0][2][3]
    # (a part's slabs take splits * k*r*s*C * 4 bytes: what unit_conv2d_wgrad_workspace_bytes returns)
    per = [passes * lib().unit_conv2d_wgrad_splits(code, n, oh, ow, k, r, s, c) for _, _, (n, _, _, _, oh, ow), passes, code in parts]
    one = k * r * s * c * 4
    slab = _fit_slab(slab, sum(per) * one, parts[0][0].device)
    at = 0
    for part, sp in zip(parts, per):
        _wgrad_launch(part, k, r, s, stride, pad, part[1].shape[-1], None, None, False, variant, slab[at * one:] if at else slab)
        at += sp
    return slab, at


# ------------------------------------------------------------------------------------------------ ragged batches (two image groups)
class Ragged:
    """Activations of TWO image groups -- the supervised and the weak batch of a training step, each zero-padded to its own largest image
    (meta_arch/rcnn.py:438-452) -- as ONE tensor: the pixel rows of group 0 followed by those of group 1, `flat` [M0 + M1, C] (plain or X3).
    Pointwise stride-1 layers run over `flat` as one GEMM (rows are independent); every other layer runs both groups in one PAIR launch
    (unit_conv2d_fwd_pair) on the group views; weight gradients take the groups as parts of one layer. `group(i)` is a zero-copy
    [n, h, w, C] view."""

    def __init__(self, flat, dims):
        assert flat.dim() == 2 and len(dims) == 2 and sum(n * h * w for n, h, w in dims) == flat.shape[0], (flat.shape, dims)
        self.flat, self.dims = flat, [tuple(d) for d in dims]

    @property
    def dtype(self):
        return self.flat.dtype

    @property
    def device(self):
        return self.flat.device

    @property
    def channels(self):
        return self.flat.shape[1]

    def rows(self, i):
        lo = 0 if i == 0 else self.dims[0][0] * self.dims[0][1] * self.dims[0][2]
        n, h, w = self.dims[i]
        return lo, lo + n * h * w

    def group(self, i):
        lo, hi = self.rows(i)
        n, h, w = self.dims[i]
        return self.flat[lo:hi].view(n, h, w, self.flat.shape[1])

    def groups(self):
        return self.group(0), self.group(1)

    def as_gemm(self):
        """[1, 1, M0 + M1, C]: what a pointwise stride-1 layer sees"""
        return self.flat.view(1, 1, self.flat.shape[0], self.flat.shape[1])

    def like(self, flat):
        return Ragged(flat, self.dims)

    def record_stream(self, stream):
        self.flat.record_stream(stream)

    @staticmethod
    def empty(dims, c, like):
        """uninitialised Ragged of `c` channels with the dtype / device / X3-ness of the tensor `like`"""
        m = sum(n * h * w for n, h, w in dims)
        t = torch.empty((m, c), dtype=like.dtype, device=like.device)
        return Ragged(t.as_subclass(X3) if type(like) is X3 else t, dims)

    @staticmethod
    def zeros(dims, c, like):
        m = sum(n * h * w for n, h, w in dims)
        t = zeros((m, c), like.dtype, like.device)
        return Ragged(t.as_subclass(X3) if type(like) is X3 else t, dims)


class Parts(tuple):
    """the operand of a layer's weight gradient as several PARTS (the image groups of an ops.Ragged through a non-pointwise layer): x = Parts of
    [n, h, w, C] tensors, dy = Parts of the matching [n, oh, ow, K] tensors. The parts' split-M slabs follow each other in the layer's buffer and
    one reduction adds them -- a part is to the weight gradient what one more split-M range is."""

    def record_stream(self, stream):
        for t in self:
            t.record_stream(stream)


class ConvSecond(ctypes.Structure):
    """include/unit_hip.h: UnitConvSecond"""
    _fields_ = [("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("residual", ctypes.c_void_p), ("mask_ref", ctypes.c_void_p)] + \
               [(f, ctypes.c_int) for f in ("N", "H", "W", "OHf", "OWf")]


def conv2d_pair(xs, w, k, r, s, stride=1, pad=0, bias=None, residuals=None, mask_refs=None, relu=False, outs=None, scatters=None, force=None):
    """the same conv layer over TWO inputs of different map sizes in ONE launch (unit_conv2d_fwd_pair; csrc/conv_epilogue.h ConvSecond):
    xs = (x0, x1) NHWC of one dtype / channel count (plain or X3), residuals / mask_refs / outs / scatters pairs (or None). The kernel and
    tile are chosen for the SUM of the two problems' pixels (force = (kernel, tile) of unit_conv2d_fwd_pair overrides: tests). Returns (y0, y1);
    each equals the single launch's result bit for bit."""
    x0, x1 = xs
    x3 = type(x0) is X3
    assert (type(x1) is X3) == x3 and x0.dtype == x1.dtype and x0.shape[3] == x1.shape[3]
    c = x0.shape[3]
    residuals = residuals or (None, None)
    mask_refs = mask_refs or (None, None)
    scatters = scatters or (None, None)
    geo = [_conv_geometry(x, r, s, stride, pad, sc) for x, sc in zip(xs, scatters)]
    assert geo[0][5] == geo[1][5], "conv2d_pair: one scatter multiplier for both problems"
    ldy = k if x3 else (k + 3) // 4 * 4
    if outs is None:
        outs = tuple(_conv_out(g, ldy, x0.dtype, x0.device, scatters[0] is not None, x3) for g in geo)
    ptr = (lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())) if x3 else _p
    if x3:
        for t in tuple(xs) + tuple(outs) + tuple(q for q in residuals + mask_refs if q is not None):
            assert type(t) is X3 and t.is_contiguous()
    m_tot = sum(g[0] * g[3] * g[4] for g in geo)
    mask_c = mask_refs[0].shape[-1] if (x3 and mask_refs[0] is not None) else 0
    if force is not None:
        kernel, tile = force
    elif x3:
        segs = w.shape[-1] // c          # (conv2d_x3)
        assert segs in (2, 3) and w.shape[-1] == segs * c
        kernel, tile = (3 if segs == 3 else 4), X3_TILE_POLICY(m_tot, k, c, segs * r * s * c)
    else:
        big, mid = select_conv_kernel(x0.dtype, m_tot, k, c, r * s * c, x0.dtype, ldy, pair=True)
        kernel, tile = (2, 0) if big else ((1, mid) if mid >= 0 else (0, 0))
    g0, g1 = geo
    sec = ConvSecond()
    sec.x, sec.y = xs[1].data_ptr(), outs[1].data_ptr()
    sec.residual = residuals[1].data_ptr() if residuals[1] is not None else None
    sec.mask_ref = mask_refs[1].data_ptr() if mask_refs[1] is not None else None
    sec.N, sec.H, sec.W, sec.OHf, sec.OWf = g1[0], g1[1], g1[2], g1[6], g1[7]
    with _timed(_conv_timed_name(kernel == 2 or (kernel in (3, 4) and tile < 0), kernel in (1, 3, 4)),
                ((3 if kernel == 3 else 2) if x3 else 1) * 2.0 * m_tot * k * r * s * c, (sum(x.numel() for x in xs) + m_tot * ldy) * x0.element_size()):
        check(lib().unit_conv2d_fwd_pair(kernel, ptr(xs[0]), _p(w), ptr(outs[0]), _p(bias), ptr(residuals[0]), ptr(mask_refs[0]), mask_c,
                                         BF16 if x3 else dt(x0.dtype), BF16 if x3 else dt(x0.dtype), g0[0], g0[1], g0[2], c, k, r, s, stride, pad, g0[3], g0[4],
                                         ldy, g0[5], g0[6], g0[7], int(relu), int(tile), ctypes.byref(sec), _s()), "unit_conv2d_fwd_pair")
    return outs


# ------------------------------------------------------------------------------------------------ bf16x3 (split) convolutions
def x3_tile_policy(m, k, c, kgemm_v):
    """kernel / tile of a bf16x3 conv with m output pixels, k filters, c real input channels, kgemm_v = 3 * r * s * c virtual k extent:
    -1 = the 256x256 phase-interleaved kernel, 0 / 1 / 2 = 4-wave tiles, >= 100 = loader / consumer tile code (the plain bf16 policies
    applied to the three times longer contraction)"""
    # (at least 200 tiles: the res4 256 -> 1024 layers -- 152 tiles on 256 CUs, 36.7 us -- run faster on the loader / consumer tiles: 36.2;
    #  tools/x3_conv_sweep.py)
    if k >= 256 and kgemm_v >= 512 and ((m + 255) // 256) * ((k + 255) // 256) >= 200:
        return -1
    if k <= 64:
        return 2
    tiles = ((m + 127) // 128) * ((k + 127) // 128)
    if kgemm_v >= 512 and tiles <= 640 and k % 8 == 0:
        return lc_tile_code(m, k, kgemm_v)
    return _four_wave_tile(m, k)


X3_TILE_POLICY = x3_tile_policy


def conv2d_x3(x, w, k, r, s, stride=1, pad=0, bias=None, residual=None, mask_ref=None, relu=False, out=None, scatter=None, tile=None):
    """bf16x3 convolution (unit_conv2d_fwd_x3): x X3 [N,H,W,C], w = weight_prep_x3's forward (or dgrad) copy, residual / mask_ref X3;
    returns an X3 [N,OH,OW,k] (or writes the strided scatter target)."""
    c = x.shape[3]
    assert x.is_contiguous() and c % 64 == 0 and k % 8 == 0, "conv2d_x3: C % 64 == 0, K % 8 == 0"
    geo = n, h, wd, oh, ow, oy_mul, ohf, owf = _conv_geometry(x, r, s, stride, pad, scatter)
    if out is None:
        out = _conv_out(geo, k, torch.float32, x.device, scatter is not None, x3=True)
    assert type(out) is X3 and out.is_contiguous()
    if residual is not None:
        assert type(residual) is X3 and residual.is_contiguous() and residual.shape[-1] == k
    mask_c = 0
    if mask_ref is not None:
        assert type(mask_ref) is X3 and mask_ref.is_contiguous()
        mask_c = mask_ref.shape[-1]
    m = n * oh * ow
    segs = w.shape[-1] // c          # 3 = [Wh | Wh | Wl]; 2 = [Wh | Wl], the two-segment dgrad copy (weight_prep_x3 dgrad_segs)
    assert segs in (2, 3) and w.shape[-1] == segs * c, "conv2d_x3: w is a weight_prep_x3 copy"
    if tile is None:
        pkey = ("x3", m, k, c, r * s, X3_TILE_POLICY, segs)
        tile = _POLICY_CACHE.get(pkey)
        if tile is None:
            tile = _POLICY_CACHE[pkey] = X3_TILE_POLICY(m, k, c, segs * r * s * c)
    # flops = the MFMA work issued: three (dgrad with two segments: two) bf16 products per fp32 product
    with _timed(_conv_timed_name(tile < 0, True), segs * 2.0 * m * k * r * s * c) as t:
        check(lib().unit_conv2d_fwd_x3s(_px(x), _p(w), _px(out), _p(bias), _px(residual), _px(mask_ref), mask_c, n, h, wd, c, k, r, s, stride, pad,
                                        oh, ow, k, oy_mul, ohf, owf, int(relu), int(tile), segs, _s()), "unit_conv2d_fwd_x3s")
        if t.prof is not None:
            t.nbytes = (x.numel() + m * k * (1 + (residual is not None))) * 4 + (m * k * 2 if mask_ref is not None else 0) + w.numel() * 2
            if tile >= 0:
                bm, bn = mid_tile_dims(tile)
                tiles = ((m + bm - 1) // bm) * ((k + bn - 1) // bn)
                t.ref_bytes = ((tiles + 255) // 256) * (segs * r * s * c // 64) * (bm + bn) * 128.0
    return out


# k-segments of the DGRAD copies of the bf16x3 mode (round 6): 2 = [Wh | Wl] against the gradient map's hi plane (dx = hi(dy).(Wh + Wl)),
# 3 = the forward's three products. UNIT_X3_DGRAD_SEGS=3 restores round 5 (A/B; profiles/r06_exp_x3_wgrad_passes.txt)
X3_DGRAD_SEGS = int(os.environ.get("UNIT_X3_DGRAD_SEGS", "2"))
assert X3_DGRAD_SEGS in (2, 3)


def weight_prep_x3(w_krsc, scale, k, r, s, c, want_fwd=True, want_dgrad=True, w_fwd=None, w_dgrad=None):
    """fp32 [k][r][s][c] storage -> (bf16 [k][r][s][c/64][3][64], bf16 [c][r][s][k/64][3][64]) = the k-segments [Wh | Wh | Wl] of the bf16x3
    convs (forward: c % 64 == 0; dgrad: k % 64 == 0; either may be skipped)"""
    dev = w_krsc.device
    if want_fwd and w_fwd is None:
        w_fwd = torch.empty((k, r, s, 3 * c), dtype=torch.bfloat16, device=dev)
    dsegs = X3_DGRAD_SEGS
    if want_dgrad and (w_dgrad is None or w_dgrad.shape[-1] != dsegs * k):
        w_dgrad = torch.empty((c, r, s, dsegs * k), dtype=torch.bfloat16, device=dev)
    check(lib().unit_weight_prep_x3s(_p(w_krsc), _p(scale), k, r, s, c, _p(w_fwd) if want_fwd else None, _p(w_dgrad) if want_dgrad else None,
                                     dsegs, _s()), "weight_prep_x3s")
    return (w_fwd if want_fwd else None), (w_dgrad if want_dgrad else None)


def _x3v(variant):
    """`variant` of unit_conv2d_wgrad_x3 with the pass count in bits 8-9 (0 = all three)"""
    return int(variant) | ((X3_WGRAD_PASSES if X3_WGRAD_PASSES != 3 else 0) << 8)


def conv2d_wgrad_x3(x, dy, k, r, s, stride=1, pad=0, scale=None, out=None, accumulate=False, variant=0, slab=None):
    """bf16x3 weight gradient: x X3 [N,H,W,C], dy X3 [N,OH,OW,k] -> dw fp32 [k,r,s,C] (scale[k] folded); the slabs alone:
    conv2d_wgrad_partial"""
    assert type(x) is X3
    return conv2d_wgrad(x, dy, k, r, s, stride, pad, scale=scale, out=out, accumulate=accumulate, variant=variant)


class WgradProblem(ctypes.Structure):
    """include/unit_hip.h: UnitWgradProblem"""
    _fields_ = [("x", ctypes.c_void_p), ("dy", ctypes.c_void_p), ("partial", ctypes.c_void_p)] + \
               [(f, ctypes.c_int) for f in ("N", "H", "W", "C", "K", "R", "S", "stride", "pad", "OH", "OW", "ldy", "splits", "kind",
                                            "x_pitch", "x_back", "dy_back")]


def wgrad_group_supported(x, dy, k, r, s, stride, pad):
    """may this layer's weight gradient go into a grouped launch (csrc/conv_wgrad128r.hip)? bf16 tensors, or X3 split tensors (each of
    the three plane passes of a bf16x3 weight gradient is a bf16 problem of its own in the grid); ops.Parts: every part"""
    return all((type(xp) is not X3 or type(dp) is X3) and bool(lib().unit_conv2d_wgrad_group_supported(code, n, oh, ow, k, r, s, c))
               for xp, dp, (n, _, _, c, oh, ow), _, code in _wgrad_parts(x, dy, k, r, s, stride, pad))


_X3_PASSES = ((0, 0), (0, 1), (1, 0))          # (plane of x, plane of dy) per pass: hi^T.hi + hi^T.lo + lo^T.hi
# How many of those passes a bf16x3 WEIGHT gradient runs (round 6). 3 = fp32-grade products (round 5). 1 = the hi planes only: every
# product is a bf16 x bf16 product of the ROUNDED operands, accumulated in fp32 over the >= 2 394 pixel rows of the contraction -- the
# forward and the dgrad chain (what the losses, the index decisions and every upstream gradient depend on) keep all three products. The
# parity tests hold weight gradients to 2e-3 of a tensor's largest entry, and what moves them at fp32-grade precision already is ReLU masks
# flipping within rounding of zero (1.6e-3, profiles/r05_fullsize_parity_metrics.json); a 2^-9 relative rounding of the operands averages
# out over the contraction. UNIT_X3_WGRAD_PASSES=3 restores the three passes (A/B; profiles/r06_exp_x3_wgrad_passes.txt).
X3_WGRAD_PASSES = int(os.environ.get("UNIT_X3_WGRAD_PASSES", "1"))
assert X3_WGRAD_PASSES in (1, 3)


def conv2d_wgrad_group(items, slabs=None, splits_hint=0):
    """split-M partial slabs of SEVERAL layers from one launch (unit_conv2d_wgrad_group). items: [(x, dy, k, r, s, stride, pad)];
    slabs: per item a uint8 tensor to reuse or None. Returns [(slab, n_splits)]; slab i of a layer = floats [i*k*r*s*C, ...) as
    conv2d_wgrad_partial leaves them. An item is one or more PROBLEMS of the grid whose slabs follow each other in the layer's buffer
    (n_splits = all of them): one per part of an ops.Parts operand (the image groups of a ragged batch), times one per plane pass for X3
    (bf16x3 split) tensors."""
    n_items = len(items)
    if n_items == 0:
        return []
    assert ctypes.sizeof(WgradProblem) == lib().unit_wgrad_problem_bytes()
    probs = []          # (item index, x part, dy part, geometry, pass | None)
    for i, it in enumerate(items):
        for xp, dp, geo, passes, _ in _wgrad_parts(*it):
            if type(xp) is X3:
                assert type(dp) is X3 and dp.shape[-1] == it[2]
                probs += [(i, xp, dp, geo, ps) for ps in range(passes)]
            else:
                probs.append((i, xp, dp, geo, None))
    pr = (WgradProblem * len(probs))()
    flops = nbytes = 0
    one = [None] * n_items          # per item: (bytes of one slab, device)
    for q, (i, x, dy, (n, h, wd, c, oh, ow), ps) in zip(pr, probs):
        _, _, k, r, s, stride, pad = items[i]
        one[i] = (k * r * s * c * 4, x.device)
        q.N, q.H, q.W, q.C, q.K, q.R, q.S, q.stride, q.pad, q.OH, q.OW = n, h, wd, c, k, r, s, stride, pad, oh, ow
        if ps is None:
            q.x, q.dy, q.ldy = x.data_ptr(), dy.data_ptr(), dy.shape[-1]
            q.x_pitch = q.x_back = q.dy_back = 0
        else:
            px, pd = _X3_PASSES[ps]
            q.x, q.dy, q.ldy = x.data_ptr() + px * c * 2, dy.data_ptr() + pd * k * 2, 2 * k
            q.x_pitch, q.x_back, q.dy_back = 2 * c, px * c, pd * k
        nbytes += (x.numel() + n * oh * ow * dy.shape[-1]) * 2 + 4 * k * r * s * c          # (X3: one bf16 plane of each operand per pass)
        flops += 2.0 * n * oh * ow * k * r * s * c
    check(lib().unit_conv2d_wgrad_group_plan(pr, len(probs), int(splits_hint)), "unit_conv2d_wgrad_group_plan")
    total = [0] * n_items
    for q, p in zip(pr, probs):
        total[p[0]] += q.splits
    out = [(_fit_slab(slabs[i] if slabs is not None else None, total[i] * one[i][0], one[i][1]), total[i]) for i in range(n_items)]
    at = [0] * n_items
    for q, p in zip(pr, probs):
        i = p[0]
        q.partial = out[i][0].data_ptr() + at[i] * one[i][0]
        at[i] += q.splits
    with _timed("conv_wgrad", flops, nbytes):
        check(lib().unit_conv2d_wgrad_group(pr, len(probs), dt(torch.bfloat16), _s()), "unit_conv2d_wgrad_group")
    return out


def frozen_bn_fold(weight, bias, running_mean, running_var, eps=1e-5):
    c = weight.numel()
    scale = torch.empty(c, dtype=torch.float32, device=weight.device)
    shift = torch.empty(c, dtype=torch.float32, device=weight.device)
    check(lib().unit_frozen_bn_fold(_p(weight), _p(bias), _p(running_mean), _p(running_var), eps, _p(scale), _p(shift), c, _s()),
          "frozen_bn_fold")
    return scale, shift


def weight_prep(w_krsc, scale, k, r, s, c, cp, dtype, want_dgrad=True, w_fwd=None, w_dgrad=None):
    """w_krsc: fp32 storage in [k][r][s][c] order (channels_last view of the [k,c,r,s] parameter)."""
    dev = w_krsc.device
    if w_fwd is None:
        w_fwd = torch.empty((k, r, s, cp), dtype=dtype, device=dev)
    if want_dgrad and w_dgrad is None:
        w_dgrad = torch.empty((c, r, s, k), dtype=dtype, device=dev)
    check(lib().unit_weight_prep(_p(w_krsc), _p(scale), k, r, s, c, cp, _p(w_fwd), _p(w_dgrad) if want_dgrad else None,
                                 dt(dtype), _s()), "weight_prep")
    return w_fwd, w_dgrad


def bias_grad(dy2d, k, out=None, accumulate=False):
    m, ld = dy2d.shape
    if out is None:
        out = torch.empty(k, dtype=torch.float32, device=dy2d.device)
    nb = lib().unit_bias_grad_scratch_bytes(m, k) if m > 1024 else 0
    ws = workspace(nb, dy2d.device, slot=3) if nb else None
    check(lib().unit_bias_grad(_p(dy2d), dt(dy2d.dtype), m, k, ld, _p(out), int(accumulate), _p(ws), nb, _s()), "bias_grad")
    return out


def linear_wgrad(x2d, dy2d, k, dw, db):
    """bf16 x [R,C], dy [R,ldy] (pad columns zero) -> dw fp32 [k,C], db fp32 [k] from one launch (csrc/linear_wgrad.hip)."""
    r, c = x2d.shape
    ldy = dy2d.shape[1]
    dev = x2d.device
    nb = lib().unit_linear_wgrad_workspace_bytes(r, c, k)
    ws = workspace(nb, dev, slot=4)
    with _timed("conv_wgrad", 2.0 * r * k * c, (x2d.numel() + r * ldy) * 2 + 4 * k * c):
        check(lib().unit_linear_wgrad(_p(x2d), _p(dy2d), dt(x2d.dtype), r, c, k, ldy, _p(dw), _p(db), _p(ws), ws.numel(), _s()),
              "unit_linear_wgrad")


def stem_conv_pool(x, w_fwd, shift, out=None):
    """bf16 x [N,H,W,8] -> [N,PH,PW,64]: 7x7 s2 conv + folded FrozenBN + ReLU + 3x3 s2 max pool in one launch (csrc/stem_pool.hip)"""
    n, h, w, c = x.shape
    assert c == 8 and tuple(w_fwd.shape) == (64, 7, 7, 8) and x.dtype == torch.bfloat16 and w_fwd.dtype == torch.bfloat16
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    ph, pw = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
    y = out if out is not None else torch.empty((n, ph, pw, 64), dtype=x.dtype, device=x.device)
    assert tuple(y.shape) == (n, ph, pw, 64) and y.is_contiguous()
    with _timed("stem", 2.0 * n * oh * ow * 64 * 147, x.numel() * 2 + y.numel() * 2):
        check(lib().unit_stem_conv_pool(_p(x), _p(w_fwd), _p(shift), _p(y), dt(x.dtype), n, h, w, _s()), "unit_stem_conv_pool")
    return y


def maxpool3x3s2(x, out=None):
    n, h, w, c = x.shape
    oh, ow = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    y = out if out is not None else torch.empty((n, oh, ow, c), dtype=x.dtype, device=x.device)
    assert tuple(y.shape) == (n, oh, ow, c) and y.is_contiguous() and y.dtype == x.dtype
    check(lib().unit_maxpool3x3s2_fwd(_p(x), _p(y), dt(x.dtype), n, h, w, c, _s()), "maxpool")
    return y


def global_avgpool(x, out=None):
    """[R,PH,PW,C] -> [R,C] (an X3 map: fp32 features, unit_global_avgpool_x3_fwd); out: contiguous rows of a larger feature matrix"""
    r, ph, pw, c = x.shape
    if out is not None:
        assert out.shape == (r, c) and out.is_contiguous() and out.dtype == (torch.float32 if type(x) is X3 else x.dtype)
    if type(x) is X3:
        y = out if out is not None else torch.empty((r, c), dtype=torch.float32, device=x.device)
        check(lib().unit_global_avgpool_x3_fwd(_px(x), _p(y), r, ph * pw, c, _s()), "avgpool_x3_fwd")
        return y
    y = out if out is not None else torch.empty((r, c), dtype=x.dtype, device=x.device)
    check(lib().unit_global_avgpool_fwd(_p(x), _p(y), dt(x.dtype), r, ph * pw, c, _s()), "avgpool_fwd")
    return y


def global_avgpool_bwd_relu(dfeat, out):
    r, ph, pw, c = out.shape
    if type(out) is X3:          # -> X3 gradient map
        g = torch.empty(out.shape, dtype=torch.float32, device=out.device).as_subclass(X3)
        check(lib().unit_global_avgpool_x3_bwd_relu(_p(dfeat), _px(out), _px(g), r, ph * pw, c, _s()), "avgpool_x3_bwd")
        return g
    g = torch.empty_like(out)
    check(lib().unit_global_avgpool_bwd_relu(_p(dfeat), _p(out), _p(g), dt(out.dtype), r, ph * pw, c, _s()), "avgpool_bwd")
    return g


# ------------------------------------------------------------------------------------------------ boxes
def cell_anchors(sizes=(32, 64, 128, 256, 512), ratios=(0.5, 1.0, 2.0)):
    """DefaultAnchorGenerator.generate_cell_anchors: python double math, then fp32."""
    out = []
    for size in sizes:
        area = size ** 2.0
        for r in ratios:
            w = math.sqrt(area / r)
            h = r * w
            out.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
    return torch.tensor(out, dtype=torch.float32)


def anchor_grid(h, w, cell, stride=16, offset=0.0):
    a = cell.shape[0]
    out = torch.empty((h * w * a, 4), dtype=torch.float32, device=cell.device)
    check(lib().unit_anchor_grid(_p(out), h, w, a, float(stride), float(offset), _p(cell), _s()), "anchor_grid")
    return out


def iou_match(gt, gt_count, boxes, box_count, thresholds, labels, allow_low_quality, want_vals=True):
    """gt [B,Mcap,4]; boxes [Ncap,4] (shared) or [B,Ncap,4]; counts: device int32 [B] or None."""
    b, mcap = gt.shape[0], gt.shape[1]
    shared = boxes.dim() == 2
    ncap = boxes.shape[-2]
    dev = gt.device
    idx = torch.empty((b, ncap), dtype=torch.int64, device=dev)
    lab = torch.empty((b, ncap), dtype=torch.int8, device=dev)
    val = torch.empty((b, ncap), dtype=torch.float32, device=dev) if want_vals else None
    th = (ctypes.c_float * len(thresholds))(*thresholds)
    lb = (ctypes.c_int * len(labels))(*labels)
    nb = lib().unit_iou_match_workspace_bytes(b, mcap)
    ws = workspace(nb, dev)
    check(lib().unit_iou_match(_p(gt), _p(gt_count), b, mcap, _p(boxes), 0 if shared else ncap * 4, _p(box_count), ncap,
                               th, lb, len(thresholds), int(allow_low_quality), _p(idx), _p(lab), _p(val), _p(ws), ws.numel(),
                               _s()), "iou_match")
    return idx, lab, val


def pairwise_iou(b1, b2):
    out = torch.empty((b1.shape[0], b2.shape[0]), dtype=torch.float32, device=b1.device)
    check(lib().unit_pairwise_iou(_p(b1), b1.shape[0], _p(b2), b2.shape[0], _p(out), _s()), "pairwise_iou")
    return out


def match_matrix(q, thresholds, labels, allow_low_quality):
    """Matcher.__call__ on an [M,N] quality matrix (modeling/matcher.py:54-98) -> (idx int64, label int8, val fp32)"""
    m, n = q.shape
    dev = q.device
    idx = torch.empty((n,), dtype=torch.int64, device=dev)
    lab = torch.empty((n,), dtype=torch.int8, device=dev)
    val = torch.empty((n,), dtype=torch.float32, device=dev)
    ws = torch.empty((max(m, 1),), dtype=torch.float32, device=dev)
    th = (ctypes.c_float * len(thresholds))(*thresholds)
    lb = (ctypes.c_int * len(labels))(*labels)
    check(lib().unit_match_matrix(_p(q.contiguous()), m, n, th, lb, len(thresholds), int(allow_low_quality), _p(idx), _p(lab), _p(val),
                                  _p(ws), _s()), "match_matrix")
    return idx, lab, val


def subsample_labels(labels, count, perm, num_samples, positive_fraction, bg_label, want_labels=True, want_idx=True):
    """labels [B,Ncap] int8|int64 ; perm [B,Pcap] int32 -> (out_labels int8 [B,Ncap], sampled_idx int32 [B,S], counts [B,2])"""
    b, ncap = labels.shape
    dev = labels.device
    out_labels = torch.empty((b, ncap), dtype=torch.int8, device=dev) if want_labels else None
    sidx = torch.empty((b, num_samples), dtype=torch.int32, device=dev) if want_idx else None
    counts = torch.empty((b, 2), dtype=torch.int32, device=dev)
    max_pos = int(num_samples * positive_fraction)
    check(lib().unit_subsample_labels(_p(labels), int(labels.dtype == torch.int64), _p(count), b, ncap, _p(perm), perm.shape[1],
                                      num_samples, max_pos, bg_label, _p(out_labels), _p(sidx), _p(counts), _s()),
          "subsample_labels")
    return out_labels, sidx, counts


def random_permutations(b, n, seed, counter, stream_id, device):
    """-> int32 [b, n]: one uniformly random permutation of range(n) per row, drawn from (seed, *counter, stream_id) by
    unit_perm_keys + the stable descending sort (replaces torch.randperm in the step; `counter` is a device int64 scalar)"""
    keys = torch.empty((b, n), dtype=torch.float32, device=device)
    check(lib().unit_perm_keys(int(seed) & 0xFFFFFFFFFFFFFFFF, _p(counter), int(stream_id), b, n, _p(keys), _s()), "perm_keys")
    _, idx = sort_desc(keys, b, n, topk=n)        # chip-wide select + rank form (the plain form is one workgroup per row)
    return idx


def counter_bump(counter, delta=1):
    check(lib().unit_counter_bump(_p(counter), int(delta), _s()), "counter_bump")


def box_encode(src, tgt, weights):
    out = torch.empty_like(src)
    w = (ctypes.c_float * 4)(*weights)
    check(lib().unit_box_encode(_p(src), _p(tgt), w, _p(out), src.shape[0], _s()), "box_encode")
    return out


def box_decode(deltas, boxes, weights, k=None, col0=0):
    n, ld = deltas.shape
    k = k or (ld - col0) // 4
    out = torch.empty((n, k * 4), dtype=torch.float32, device=deltas.device)
    w = (ctypes.c_float * 4)(*weights)
    check(lib().unit_box_decode(_p(deltas), ld, col0, k, _p(boxes), w, SCALE_CLAMP, _p(out), n, _s()), "box_decode")
    return out


def sort_desc(src, b, n, ld=1, a=1, col0=0, batch_stride=None, topk=None, min_exclusive=None):
    """stable descending sort of n keys per batch row; keys read as src[b*bstride + (i//a)*ld + col0 + i%a].
    topk: only the first min(topk, n) entries of each output row are needed (chip-wide select + rank sort);
    min_exclusive (with topk): keys <= it are not ranked at all (rows are defined up to the number of larger keys)."""
    dev = src.device
    keys = torch.empty((b, n), dtype=torch.float32, device=dev)
    idx = torch.empty((b, n), dtype=torch.int32, device=dev)
    if batch_stride is None:
        batch_stride = (n // a) * ld
    nb = lib().unit_sort_workspace_bytes(b, n)
    ws = workspace(nb, dev)
    if topk is not None:
        with _timed("sort_topk", 0.0, b * n * 4.0):
            check(lib().unit_sort_desc_stable_topk(_p(src), batch_stride, ld, a, col0, b, n, int(topk),
                                                   float("-inf") if min_exclusive is None else float(min_exclusive), _p(keys), _p(idx),
                                                   _p(ws), ws.numel(), _s()), "sort_desc_stable_topk")
        return keys, idx
    check(lib().unit_sort_desc_stable(_p(src), batch_stride, ld, a, col0, b, n, _p(keys), _p(idx), _p(ws), ws.numel(), _s()),
          "sort_desc_stable")
    return keys, idx


def rpn_decode_select(head, a, delta_col0, anchors, sorted_idx, sorted_logit, topk, image_hw, min_size=0.0):
    """head [B,HW,ld] fp32 -> (cand_boxes [B,topk,4], cand_scores [B,topk], cand_count [B])"""
    b, hw, ld = head.shape
    ncap = anchors.shape[0]
    dev = head.device
    cb = torch.empty((b, topk, 4), dtype=torch.float32, device=dev)
    cs = torch.empty((b, topk), dtype=torch.float32, device=dev)
    cc = torch.empty((b,), dtype=torch.int32, device=dev)
    check(lib().unit_rpn_decode_select(_p(head), hw * ld, ld, a, delta_col0, _p(anchors), _p(sorted_idx), _p(sorted_logit), b, ncap,
                                       topk, _p(image_hw), SCALE_CLAMP, float(min_size), _p(cb), _p(cs), _p(cc), _s()),
          "rpn_decode_select")
    return cb, cs, cc


def nms(boxes_sorted, scores_sorted, count, thresh, max_keep, out=None):
    """boxes [B,cap,4] in descending score order -> (keep_idx [B,max_keep], keep_count [B], out_boxes, out_scores).
    out = (boxes [B,max_keep,4], scores [B,max_keep], keep_count int32 [B]): rows of larger buffers to write into (a two-pass step keeps the
    proposals of both passes in one tensor)"""
    b, cap = boxes_sorted.shape[0], boxes_sorted.shape[1]
    dev = boxes_sorted.device
    keep = torch.empty((b, max_keep), dtype=torch.int32, device=dev)      # unit_nms writes the tails (-1 / 0) itself
    if out is not None:
        ob, osc, kc = out
        assert ob.shape == (b, max_keep, 4) and osc.shape == (b, max_keep) and kc.shape == (b,) and ob.is_contiguous() and osc.is_contiguous()
    else:
        kc = torch.empty((b,), dtype=torch.int32, device=dev)
        ob = torch.empty((b, max_keep, 4), dtype=torch.float32, device=dev)
        osc = torch.empty((b, max_keep), dtype=torch.float32, device=dev)
    nb = lib().unit_nms_workspace_bytes(b, cap)
    ws = workspace(nb, dev)
    with _timed("nms", 0.0, b * cap * 20.0):
        check(lib().unit_nms(_p(boxes_sorted), _p(scores_sorted), _p(count), b, cap, float(thresh), max_keep, _p(keep), _p(kc), _p(ob),
                             _p(osc), _p(ws), ws.numel(), _s()), "nms")
    return keep, kc, ob, osc


# ------------------------------------------------------------------------------------------------ a7 plumbing
def append_gt(props, pcount, gt, gcount):
    b, pcap = props.shape[0], props.shape[1]
    mcap = gt.shape[1]
    cat = torch.empty((b, pcap + mcap, 4), dtype=torch.float32, device=props.device)
    cc = torch.empty((b,), dtype=torch.int32, device=props.device)
    check(lib().unit_append_gt(_p(props), _p(pcount), pcap, _p(gt), _p(gcount), mcap, b, _p(cat), _p(cc), _s()), "append_gt")
    return cat, cc


def roi_classes(match_idx, match_label, count, gt_classes, gcount, k):
    b, ncap = match_idx.shape
    cls = torch.empty((b, ncap), dtype=torch.int64, device=match_idx.device)
    check(lib().unit_roi_classes(_p(match_idx), _p(match_label), _p(count), _p(gt_classes), _p(gcount), gt_classes.shape[1], b, ncap,
                                 k, _p(cls), _s()), "roi_classes")
    return cls


def gather_rois(cat, sampled_idx, cls, match_idx, gt, gcount, rois_out=None):
    """rois_out: [b * s, 5] fp32 rows of a larger buffer to write the RoIs into (the step keeps supervised and weak RoIs in one tensor)"""
    b, ncap = cat.shape[0], cat.shape[1]
    s = sampled_idx.shape[1]
    dev = cat.device
    rois = rois_out if rois_out is not None else torch.empty((b * s, 5), dtype=torch.float32, device=dev)
    assert rois.shape == (b * s, 5) and rois.is_contiguous()
    rcls = torch.empty((b * s,), dtype=torch.int32, device=dev)
    rgt = torch.empty((b * s, 4), dtype=torch.float32, device=dev)
    check(lib().unit_gather_rois(_p(cat), ncap, _p(sampled_idx), s, _p(cls), _p(match_idx), _p(gt), _p(gcount), gt.shape[1], b,
                                 _p(rois), _p(rcls), _p(rgt), _s()), "gather_rois")
    return rois, rcls, rgt


def first_k_rois(props, pcount, s, batch_index_offset=0, rois_out=None):
    b, pcap = props.shape[0], props.shape[1]
    rois = rois_out if rois_out is not None else torch.empty((b * s, 5), dtype=torch.float32, device=props.device)
    assert rois.shape == (b * s, 5) and rois.is_contiguous()
    valid = torch.empty((b * s,), dtype=torch.int32, device=props.device)
    check(lib().unit_first_k_rois(_p(props), _p(pcount), pcap, s, b, batch_index_offset, _p(rois), _p(valid), _s()), "first_k_rois")
    return rois, valid


# ------------------------------------------------------------------------------------------------ a8
def roi_align(feat, rois, pooled_size=14, out_size=None, bin_step=1, spatial_scale=1.0 / 16, sampling_ratio=0, aligned=True,
              roi_count=None, out=None, image_offset=0):
    """image_offset: the RoIs' batch indices count from `image_offset` (feat[0] is image `image_offset` of the step's batch: the weak images
    of a two-pass step). The kernel addresses image b at base + b * H * W * C, so the base handed over is moved back by that many images."""
    n, h, w, c = feat.shape
    r = rois.shape[0]
    out_size = out_size or pooled_size
    if out is None:
        out = torch.empty((r, out_size, out_size, c), dtype=feat.dtype, device=feat.device)
    # algorithmic bytes: the maps once + the pooled tensor once; `ref` = the reference-equivalent full 14x14 output
    es = feat.element_size()
    # ref_bytes: what the reference's ROIAlignV2 call moves for the same RoIs -- the full pooled_size x pooled_size grid (roi_heads.py:499:
    # 14 x 14), of which the strided mode materialises only the bins Res5's stride-2 1x1 convs read
    with _timed("roi_align_fwd", 0.0, (feat.numel() + r * out_size * out_size * c) * es, (feat.numel() + r * pooled_size * pooled_size * c) * es):
        _p(feat)
        base = ctypes.c_void_p(feat.data_ptr() - image_offset * h * w * c * es)
        check(lib().unit_roi_align_fwd(base, dt(feat.dtype), n + image_offset, h, w, c, _p(rois), _p(roi_count), r, pooled_size, out_size, bin_step,
                                       float(spatial_scale), sampling_ratio, int(aligned), _p(out), _s()), "roi_align_fwd")
    return out


def roi_align_bwd(gout, feat_shape, rois, dfeat32=None, pooled_size=14, bin_step=1, spatial_scale=1.0 / 16, sampling_ratio=0,
                  aligned=True, roi_count=None):
    n, h, w, c = feat_shape
    r, out_size = gout.shape[0], gout.shape[1]
    if dfeat32 is None:
        dfeat32 = torch.zeros((n, h, w, c), dtype=torch.float32, device=gout.device)
    check(lib().unit_roi_align_bwd(_p(gout), dt(gout.dtype), n, h, w, c, _p(rois), _p(roi_count), r, pooled_size, out_size, bin_step,
                                   float(spatial_scale), sampling_ratio, int(aligned), _p(dfeat32), _s()), "roi_align_bwd")
    return dfeat32


def roi_align_bwd_gather(gout, n_images, h, w, rois, out, pooled_size=14, bin_step=1, spatial_scale=1.0 / 16, sampling_ratio=0,
                         aligned=True, rois_per_image=0, image_offset=0, addend=None, addend_images=0, mask_ref=None, roi_count=None):
    """deterministic gather-form RoIAlign backward; `out` [n_images,h,w,C] (fp32 or gout.dtype) is fully overwritten with
    cast((sum_of_roi_contributions [+ addend]) [* (mask_ref > 0)])."""
    r, out_size, c = gout.shape[0], gout.shape[1], gout.shape[3]
    nb = lib().unit_roi_align_bwd_gather_workspace_bytes(r)
    ws = workspace(nb, gout.device, slot=1)
    nb_alg = gout.numel() * gout.element_size() + out.numel() * out.element_size() * (1 + (addend is not None) + (mask_ref is not None))
    with _timed("roi_align_bwd_gather", 0.0, nb_alg, nb_alg + (pooled_size * pooled_size - out_size * out_size) * r * c * gout.element_size()):
        check(lib().unit_roi_align_bwd_gather(_p(gout), dt(gout.dtype), n_images, h, w, c, _p(rois), _p(roi_count), r, rois_per_image,
                                              image_offset, pooled_size, out_size, bin_step, float(spatial_scale), sampling_ratio,
                                              int(aligned), _p(addend), addend_images, _p(mask_ref), _p(out), dt(out.dtype), _p(ws),
                                              ws.numel(), _s()), "roi_align_bwd_gather")
    return out


def roi_pool(feat, rois, pooled_size=14, out_size=None, bin_step=1, spatial_scale=1.0 / 16, roi_count=None, out=None, argmax=None,
             image_offset=0):
    """torchvision's RoIPool (csrc/roi_pool.hip) with roi_align's out_size / bin_step / image_offset. argmax: None (nothing stored) or an
    int32 tensor shaped like the output, filled with y * W + x inside the RoI's image (-1: none) -- image-local under `image_offset` too, so
    that roi_pool_bwd_gather on the same slice of the batch reads what this call wrote."""
    n, h, w, c = feat.shape
    r = rois.shape[0]
    out_size = out_size or pooled_size
    if out is None:
        out = torch.empty((r, out_size, out_size, c), dtype=feat.dtype, device=feat.device)
    assert out.shape == (r, out_size, out_size, c) and out.dtype == feat.dtype and out.is_contiguous() and feat.is_contiguous()
    if argmax is not None:
        assert argmax.shape == out.shape and argmax.dtype == torch.int32 and argmax.is_contiguous()
        assert argmax.numel() * 4 == lib().unit_roi_pool_argmax_bytes(r, out_size, c)
    es = feat.element_size()
    nb_arg = 0 if argmax is None else argmax.numel() * 4
    # algorithmic bytes as roi_align's: the maps once + the pooled tensor (+ its argmax) once; `ref` = the full pooled_size x pooled_size grid
    with _timed("roi_pool_fwd", 0.0, (feat.numel() + r * out_size * out_size * c) * es + nb_arg,
                (feat.numel() + r * pooled_size * pooled_size * c) * es + (nb_arg // (out_size * out_size)) * pooled_size * pooled_size):
        _p(feat)
        base = ctypes.c_void_p(feat.data_ptr() - image_offset * h * w * c * es)
        check(lib().unit_roi_pool_fwd(base, dt(feat.dtype), n + image_offset, h, w, c, _p(rois), _p(roi_count), r, pooled_size, out_size, bin_step,
                                      float(spatial_scale), _p(out), _p(argmax), _s()), "roi_pool_fwd")
    return out


def roi_pool_bwd_gather(gout, argmax, n_images, h, w, rois, out, pooled_size=14, bin_step=1, spatial_scale=1.0 / 16, rois_per_image=0,
                        image_offset=0, addend=None, addend_images=0, mask_ref=None, roi_count=None):
    """deterministic gather-form RoIPool backward from the forward's `argmax`; `out` [n_images,h,w,C] (fp32 or gout.dtype) is fully
    overwritten with cast((sum_of_roi_contributions [+ addend]) [* (mask_ref > 0)])."""
    r, out_size, c = gout.shape[0], gout.shape[1], gout.shape[3]
    assert argmax is not None and argmax.shape == gout.shape and argmax.dtype == torch.int32 and argmax.is_contiguous() and gout.is_contiguous()
    assert out.shape == (n_images, h, w, c) and out.is_contiguous()
    nb = lib().unit_roi_pool_bwd_gather_workspace_bytes(r)
    ws = workspace(nb, gout.device, slot=1)
    nb_alg = (gout.numel() * gout.element_size() + argmax.numel() * 4
              + out.numel() * out.element_size() * (1 + (addend is not None) + (mask_ref is not None)))
    with _timed("roi_pool_bwd_gather", 0.0, nb_alg,
                nb_alg + (pooled_size * pooled_size - out_size * out_size) * r * c * (gout.element_size() + 4)):
        check(lib().unit_roi_pool_bwd_gather(_p(gout), _p(argmax), dt(gout.dtype), n_images, h, w, c, _p(rois), _p(roi_count), r,
                                             rois_per_image, image_offset, pooled_size, out_size, bin_step, float(spatial_scale),
                                             _p(addend), addend_images, _p(mask_ref), _p(out), dt(out.dtype), _p(ws), ws.numel(), _s()),
              "roi_pool_bwd_gather")
    return out


# ------------------------------------------------------------------------------------------------ losses
BOX_LOSS_TYPES = {"smooth_l1": 0, "giou": 1}          # include/unit_hip.h: UNIT_BOXLOSS_SMOOTH_L1 / UNIT_BOXLOSS_GIOU


def _box_loss_args(loss_type, beta, what):
    """(kind, beta) of the _ex loss exports, or None for Detectron2's default (smooth-L1 with beta 0 == L1): that one keeps its own export, so
    a default model's launch list is what it always was"""
    if loss_type not in BOX_LOSS_TYPES:
        raise ValueError(f"Invalid {what} loss type '{loss_type}'")
    beta = float(beta)
    if not beta >= 0.0:
        raise ValueError(f"smooth_l1_beta must be >= 0, got {beta}")
    return None if (loss_type == "smooth_l1" and beta == 0.0) else (BOX_LOSS_TYPES[loss_type], beta)


def rpn_loss(head, a, dcol0, labels, match_idx, gt_boxes, anchors, normalizer, grad_dtype, gscale=1.0, loss_out=None, weights=(1.0, 1.0),
             loss_type="smooth_l1", beta=0.0):
    """weights = (loss_rpn_cls, loss_rpn_loc) factors of Detectron2's RPN `loss_weight` (rpn.py:100); loss_type / beta = its `box_reg_loss_type`
    ("smooth_l1" | "giou") and `smooth_l1_beta` (rpn.py:68-87)"""
    ex = _box_loss_args(loss_type, beta, "rpn box reg")
    b, hw, ld = head.shape
    ncap = anchors.shape[0]
    loss2 = loss_out if loss_out is not None else torch.empty(2, dtype=torch.float32, device=head.device)
    dhead = torch.empty((b, hw, ld), dtype=grad_dtype, device=head.device)
    nbytes = lib().unit_rpn_loss_scratch_bytes(b, ncap)
    scratch = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=head.device)
    args = (_p(head), ld, a, dcol0, _p(labels), _p(match_idx), _p(gt_boxes), gt_boxes.shape[1], _p(anchors), b, ncap, float(normalizer),
            float(gscale), float(weights[0]), float(weights[1]), _p(loss2), _p(dhead), dt(grad_dtype), _p(scratch), nbytes)
    with _timed("rpn_loss"):
        if ex is None:
            check(lib().unit_rpn_loss_w(*args, _s()), "rpn_loss")
        else:
            check(lib().unit_rpn_loss_ex(*args, ex[0], ex[1], _s()), "rpn_loss_ex")
    return loss2, dhead


def sup_scores(delta, dcol0, weak, wcol0, n_oicr, ncls, novel_mask=None, extra=None, ecol0=0):
    r = delta.shape[0]
    out = torch.empty((r, ncls), dtype=torch.float32, device=delta.device)
    check(lib().unit_sup_scores(_p(delta), delta.shape[1], dcol0, _p(weak), weak.shape[1] if weak is not None else 0, wcol0, n_oicr,
                                ncls, _p(novel_mask), _p(extra), extra.shape[1] if extra is not None else 0, ecol0, _p(out), ncls, r,
                                _s()), "sup_scores")
    return out


_LOSS_ACC = {}
_MULTI_WG_LOSSES = os.environ.get("UNIT_MULTI_WG_LOSSES", "1") != "0"


def _loss_acc(device):
    """the 8-byte accumulator of the multi-workgroup loss kernels (include/unit_hip.h: unit_softmax_ce): one per (device, HIP stream), zeroed
    once -- the kernels hand it back zero, launches on a stream are ordered"""
    if not _MULTI_WG_LOSSES or device.type != "cuda":
        return None
    key = (device, raw_stream(device.index))
    a = _LOSS_ACC.get(key)
    if a is None:
        a = _LOSS_ACC[key] = zeros(2, torch.int32, device)
    elif _DEBUG_SYNC:          # diagnostic runs follow faults: a loss kernel that was aborted mid-ticket left its count behind
        check(lib().unit_fill_zero(_p(a), a.numel() * a.element_size(), _s()), "fill_zero")
    return a


def softmax_ce(logits, col0, ncls, labels, weights=None, dy=None, dcol0=0, gscale=1.0, loss_out=None):
    """weights: per-row, NON-NEGATIVE (the reference's are OICR pseudo-label scores, weak_detector_fast_rcnn.py:198-226): with more than 256
    rows the per-workgroup partial sums travel as unsigned fixed point (csrc/losses.hip packed_sum_finish), where a negative, NaN or
    >= 2^23 partial is reported as a NaN loss -- checked here under UNIT_DEBUG_SYNC=1"""
    r, ld = logits.shape
    if _DEBUG_SYNC and weights is not None and weights.numel():
        assert float(weights.min()) >= 0.0, "softmax_ce: negative row weights"
    loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=logits.device)
    check(lib().unit_softmax_ce(_p(logits), ld, col0, ncls, _p(labels), _p(weights), r, float(gscale), _p(loss), _p(dy),
                                dt(dy.dtype) if dy is not None else 0, dy.shape[1] if dy is not None else 0, dcol0, _p(_loss_acc(logits.device)),
                                _s()), "softmax_ce")
    return loss


def box_reg_loss(bbox, col0, k, labels, rois5, gt_boxes, weights, dy=None, dcol0=0, gscale=1.0, loss_out=None, loss_type="smooth_l1", beta=0.0):
    """loss_type / beta: FastRCNNOutputs' `box_reg_loss_type` ("smooth_l1" | "giou") and `smooth_l1_beta` (fast_rcnn.py:70-87)"""
    ex = _box_loss_args(loss_type, beta, "bbox reg")
    r, ld = bbox.shape
    loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=bbox.device)
    w = (ctypes.c_float * 4)(*weights)
    args = (_p(bbox), ld, col0, k, _p(labels), _p(rois5), _p(gt_boxes), w, r, float(gscale), _p(loss), _p(dy),
            dt(dy.dtype) if dy is not None else 0, dy.shape[1] if dy is not None else 0, dcol0, _p(_loss_acc(bbox.device)))
    with _timed("box_reg_loss"):
        if ex is None:
            check(lib().unit_box_reg_loss(*args, _s()), "box_reg_loss")
        else:
            check(lib().unit_box_reg_loss_ex(*args, ex[0], ex[1], _s()), "box_reg_loss_ex")
    return loss


def wsddn_mil(streams, ccol0, dcol0, k, valid, s, b, multihot, cls_temp, det_temp, mil_multiplier, dy=None, dyc0=0, dyd0=0,
              gscale=1.0, loss_out=None):
    rtot, ld = streams.shape
    loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=streams.device)
    xr = torch.empty((rtot, k), dtype=torch.float32, device=streams.device)
    check(lib().unit_wsddn_mil(_p(streams), ld, ccol0, dcol0, k, _p(valid), s, b, _p(multihot), float(cls_temp), float(det_temp),
                               float(mil_multiplier), float(gscale), _p(loss), _p(xr), _p(dy), dt(dy.dtype) if dy is not None else 0,
                               dy.shape[1] if dy is not None else 0, dyc0, dyd0, _s()), "wsddn_mil")
    return loss, xr


def max_weak_rows():
    """the most rows per image `oicr_targets(..., wide=True)` takes (unit_oicr_targets_max_rows: 8192)"""
    return int(lib().unit_oicr_targets_max_rows())


def oicr_targets(src, col0, mode, k, rois5, valid, s, b, multihot, fg_thresh=0.5, bg_thresh=0.1, want_boxes=False, wide=False):
    """want_boxes (the regression branch): -> (labels, weights, gt_boxes [b * s, 4]), the box of the pseudo-GT each row was matched to
    (unit_oicr_targets_ex); the plain form keeps its own export, so a model without the branch launches what it always did.
    wide (MODEL.LOAD_PROPOSALS): unit_oicr_targets_wide, up to max_weak_rows() rows per image instead of 1024, with or without the boxes"""
    rtot = rois5.shape[0]
    if wide and (rtot != b * s or valid.numel() != rtot or src.shape[0] != rtot or multihot.numel() != b * k):
        raise ValueError("oicr_targets: src, rois5 and valid need b * s rows, multihot b * k entries")
    labels = torch.empty((rtot,), dtype=torch.int32, device=src.device)
    weights = torch.empty((rtot,), dtype=torch.float32, device=src.device)
    args = (_p(src), src.shape[1], col0, mode, k, _p(rois5), _p(valid), s, b, _p(multihot), float(fg_thresh), float(bg_thresh), _p(labels),
            _p(weights))
    if wide:
        boxes = torch.empty((rtot, 4), dtype=torch.float32, device=src.device) if want_boxes else None
        check(lib().unit_oicr_targets_wide(*args, _p(boxes), _s()), "oicr_targets_wide")
        return (labels, weights, boxes) if want_boxes else (labels, weights)
    if not want_boxes:
        check(lib().unit_oicr_targets(*args, _s()), "oicr_targets")
        return labels, weights
    if rtot != b * s or valid.numel() != rtot or src.shape[0] != rtot:
        raise ValueError("oicr_targets: src, rois5 and valid need b * s rows")
    boxes = torch.empty((rtot, 4), dtype=torch.float32, device=src.device)
    check(lib().unit_oicr_targets_ex(*args, _p(boxes), _s()), "oicr_targets_ex")
    return labels, weights, boxes


def softmax_mean(logits, col0, step, n, k, valid=None):
    """oicr_mean_scores (weak_detector_fast_rcnn.py:248) -> [R, k + 1]: the mean over `n` refinement streams (columns col0 + t * step) of
    their row softmaxes; rows with valid < 0 are zeros (include/unit_hip.h: unit_softmax_mean)"""
    r, ld = logits.shape
    if valid is not None and valid.numel() != r:
        raise ValueError("softmax_mean: valid needs one entry per row")
    out = torch.empty((r, k + 1), dtype=torch.float32, device=logits.device)
    check(lib().unit_softmax_mean(_p(logits), ld, col0, step, n, k, _p(valid), _p(out), k + 1, r, _s()), "softmax_mean")
    return out


def pcl_loss(logits, col0, k, valid, s, b, labels, cls_weights, gt_assign, pc_count, pc_img_cls_weights, pc_probs, n_pc, dy=None, dcol0=0,
             gscale=1.0, loss_out=None):
    """PCL loss of one refinement stream (include/unit_hip.h: unit_pcl_loss): images in fixed slots of `s` rows (logits, valid, labels,
    cls_weights, gt_assign, dy: b * s rows), clusters in [b, ldc] tables (pc_count int32, pc_img_cls_weights / pc_probs fp32), n_pc int32 [b].
    Returns the loss [1]; dy gets the logits gradient in columns [dcol0, dcol0 + k + 1)."""
    r, ld = logits.shape
    rows = b * s
    if r != rows or any(t.numel() != rows for t in (valid, labels, cls_weights, gt_assign)) or (dy is not None and dy.shape[0] != rows):
        raise ValueError("pcl_loss: logits, valid, labels, cls_weights, gt_assign and dy need b * s rows")
    ldc = pc_count.shape[1] if pc_count.dim() == 2 else -1
    if any(t.dim() != 2 or tuple(t.shape) != (b, ldc) for t in (pc_count, pc_img_cls_weights, pc_probs)) or n_pc.numel() != b:
        raise ValueError("pcl_loss: cluster tables must be [b, ldc] and n_pc [b]")
    loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=logits.device)
    check(lib().unit_pcl_loss(_p(logits), ld, col0, k, _p(valid), s, b, _p(labels), _p(cls_weights), _p(gt_assign), _p(pc_count),
                              _p(pc_img_cls_weights), _p(pc_probs), _p(n_pc), ldc, float(gscale), _p(loss), _p(dy),
                              dt(dy.dtype) if dy is not None else 0, dy.shape[1] if dy is not None else 0, dcol0, _p(_loss_acc(logits.device)),
                              _s()), "pcl_loss")
    return loss


def kmeans_draws():
    """the 7 float64 draws of RandomState(3) that unit_pcl_targets carries as constants (host only)"""
    import numpy as np
    bits = (ctypes.c_ulonglong * 7)()
    check(lib().unit_kmeans_draws(bits), "kmeans_draws")
    return np.frombuffer(bytes(bits), dtype=np.float64).copy()


def pcl_targets(src, col0, mode, nxt, ncol0, nmode, k, rois5, valid, s, b, multihot, ldc, n_streams=1, step=0, nstep=0, fg_thresh=0.5,
                bg_thresh=0.1, graph_iou_thresh=0.4, max_pc_num=5, want_boxes=False):
    """PCL targets of `n_streams` refinement streams (include/unit_hip.h: unit_pcl_targets) -> dict of unit_pcl_loss's inputs, every entry
    with a leading stream axis: labels / cls_weights / gt_assign [n_streams, b * s], pc_labels / pc_count / pc_img_cls_weights / pc_probs
    [n_streams, b, ldc], n_pc [n_streams, b]. Stream t reads src columns col0 + t * step and nxt columns ncol0 + t * nstep.
    want_boxes (the regression branch): additionally gt_boxes [n_streams, b * s, 4], the centre box each row was matched to
    (unit_pcl_targets_ex); the plain form keeps its own export.
    Nothing here is a stock torch operator: torch.empty only reserves memory (the step's pool under ReplayedStep)."""
    dev, rows = src.device, b * s
    if rois5.shape[0] != rows or valid.numel() != rows or src.shape[0] != rows or nxt.shape[0] != rows:
        raise ValueError("pcl_targets: src, nxt, rois5 and valid need b * s rows")
    if multihot.numel() != b * k:
        raise ValueError("pcl_targets: multihot must be [b, k]")
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = dict(labels=i32(n_streams, rows), cls_weights=f32(n_streams, rows), gt_assign=i32(n_streams, rows), n_pc=i32(n_streams, b),
               pc_labels=i32(n_streams, b, ldc), pc_count=i32(n_streams, b, ldc), pc_img_cls_weights=f32(n_streams, b, ldc),
               pc_probs=f32(n_streams, b, ldc))
    nb = lib().unit_workspace_bytes_pcl_targets(b, s, n_streams)
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    args = (_p(src), src.shape[1], col0, mode, step, _p(nxt), nxt.shape[1], ncol0, nmode, nstep, k, _p(rois5), _p(valid),
            s, b, n_streams, _p(multihot), float(fg_thresh), float(bg_thresh), float(graph_iou_thresh), int(max_pc_num),
            _p(out["labels"]), _p(out["cls_weights"]), _p(out["gt_assign"]), _p(out["n_pc"]), _p(out["pc_labels"]),
            _p(out["pc_count"]), _p(out["pc_img_cls_weights"]), _p(out["pc_probs"]), ldc)
    if want_boxes:
        out["gt_boxes"] = f32(n_streams, rows, 4)
        check(lib().unit_pcl_targets_ex(*args, _p(out["gt_boxes"]), _p(ws), nb, _s()), "pcl_targets_ex")
    else:
        check(lib().unit_pcl_targets(*args, _p(ws), nb, _s()), "pcl_targets")
    return out


# ------------------------------------------------------------------------------------------------ a14 / a15
def embedding_similarity(emb, novel_rows, base_rows):
    """fast_rcnn.py:376-382: E[novel] @ E[base]^T (row index lists are device int32 tensors)"""
    out = torch.empty((novel_rows.numel(), base_rows.numel()), dtype=torch.float32, device=emb.device)
    check(lib().unit_embedding_similarity(_p(emb), emb.shape[1], emb.shape[1], _p(novel_rows), novel_rows.numel(), _p(base_rows),
                                          base_rows.numel(), _p(out), _s()), "embedding_similarity")
    return out


def similarity(lin_weak, col0, n_oicr, ncls, base_dev, lingual, n_novel, visual_threshold, use_lingual=True, use_visual=True):
    r = lin_weak.shape[0]
    nb = base_dev.numel()
    sim = torch.empty((r, n_novel, nb), dtype=torch.float32, device=lin_weak.device)
    check(lib().unit_similarity(_p(lin_weak), lin_weak.shape[1], col0, n_oicr, ncls, _p(base_dev), nb, _p(lingual), n_novel,
                                float(visual_threshold), int(use_lingual), int(use_visual), _p(sim), r, _s()), "similarity")
    return sim


def transfer_predictions(lin, ccol0, bcol0, k, weak, wcol0, n_oicr, sim_cls, sim_bbox, base_dev, novel_dev, role_dev, slot_dev,
                         ft=None, fccol0=0, fbcol0=0, wbcol0=None):
    """-> (scores [R,K+1], bbox [R,4K]) of SupervisedDetectorOutputs*.forward (eval / fine-tune branches).
    wbcol0: first column, in `weak`, of the weak head's [R, 4K] box deltas (REGRESSION_BRANCH under the fine-tune predictor), added to the
    transferred deltas before `ft` in the same launch (unit_transfer_predictions_ex); None: the plain entry, as every call without it records."""
    r = lin.shape[0]
    scores = torch.empty((r, k + 1), dtype=torch.float32, device=lin.device)
    bbox = torch.empty((r, 4 * k), dtype=torch.float32, device=lin.device)
    head = (_p(lin), lin.shape[1], ccol0, bcol0, k, _p(weak), weak.shape[1] if weak is not None else 0, wcol0, n_oicr)
    tail = (_p(ft), ft.shape[1] if ft is not None else 0, fccol0, fbcol0, _p(sim_cls), _p(sim_bbox), _p(base_dev), base_dev.numel(),
            _p(novel_dev), novel_dev.numel(), _p(role_dev), _p(slot_dev), _p(scores), k + 1, _p(bbox), 4 * k, r, _s())
    if wbcol0 is None:
        check(lib().unit_transfer_predictions(*head, *tail), "transfer_predictions")
    else:
        check(lib().unit_transfer_predictions_ex(*head, int(wbcol0), *tail), "transfer_predictions_ex")
    return scores, bbox


def transfer_predictions_bwd(dy, dccol0, dbcol0, lin, ccol0, bcol0, k, sim_cls, sim_bbox, t, ldl):
    """backward of transfer_predictions w.r.t. the delta heads' outputs and the similarity -> (dlin [R, ldl] in dy's dtype, dsim fp32)"""
    r = lin.shape[0]
    dlin = torch.empty((r, ldl), dtype=dy.dtype, device=lin.device)
    dsim = torch.empty(sim_cls.shape, dtype=torch.float32, device=lin.device)
    check(lib().unit_transfer_predictions_bwd(_p(dy), dt(dy.dtype), dy.shape[1], dccol0, dbcol0, _p(lin), lin.shape[1], ccol0, bcol0, k,
                                              _p(sim_cls), _p(sim_bbox), _p(t["base"]), t["base"].numel(), _p(t["novel"]), t["novel"].numel(),
                                              _p(t["role"]), _p(t["slot"]), _p(dlin), ldl, _p(dsim), r, _s()), "transfer_predictions_bwd")
    return dlin, dsim


def similarity_bwd(lin_weak, col0, n_oicr, ncls, base_dev, lingual, n_novel, visual_threshold, use_lingual, use_visual, dsim, grad_dtype):
    """backward of `similarity` -> d(loss)/d(lin_weak) [R, ld] (only the OICR logit columns are non-zero)"""
    r, ld = lin_weak.shape
    dlin = torch.empty((r, ld), dtype=grad_dtype, device=lin_weak.device)
    check(lib().unit_similarity_bwd(_p(lin_weak), ld, col0, n_oicr, ncls, _p(base_dev), base_dev.numel(), _p(lingual), n_novel,
                                    float(visual_threshold), int(use_lingual), int(use_visual), _p(dsim), _p(dlin), dt(grad_dtype), ld, col0, r,
                                    _s()), "similarity_bwd")
    return dlin


def similarity_static(w_master, row0, n_oicr, ncls, base_dev, novel_dev, lingual, plan):
    """the per-model part of a term plan (modeling/similarity_terms.Plan) -> A [n_novel, n_base] = w (softmax(lingual) + TopK + WTopK + LSDA);
    w_master: fp32 [rows, D] master matrix of the weak head's fused Linear, its refinement streams at rows row0 + s * ncls + class"""
    if w_master is None:
        raise ValueError("similarity_static: the weak head's fused Linear has no master matrix yet (LinearGroup.prepare)")
    if w_master.dtype != torch.float32 or w_master.dim() != 2 or w_master.stride(1) != 1:
        raise ValueError("similarity_static: the class weights must be a row-major fp32 matrix")
    nb, nn_ = base_dev.numel(), novel_dev.numel()
    if row0 < 0 or row0 + n_oicr * ncls > w_master.shape[0]:
        raise ValueError("similarity_static: the refinement streams' rows leave the master matrix")
    a = torch.empty((nn_, nb), dtype=torch.float32, device=w_master.device)
    check(lib().unit_similarity_static(_p(w_master), w_master.stride(0), row0, n_oicr, ncls, w_master.shape[1], _p(base_dev), nb, _p(novel_dev),
                                       nn_, _p(lingual), float(plan.weight), int(plan.lingual), plan.topk, plan.wtopk, plan.lsda, _p(a), _s()),
          "similarity_static")
    return a


def _plan_words(plan, visual_threshold):
    return (float(visual_threshold), float(plan.weight), int(plan.visual), plan.visualk, int(plan.average), int(plan.zero), int(plan.product))


def similarity_ex(lin_weak, col0, n_oicr, ncls, base_dev, a, visual_threshold, plan):
    """sim [R, n_novel, n_base] of a term plan from its static part `a` and the weak head's logits on the box features"""
    r = lin_weak.shape[0]
    nn_, nb = a.shape
    if col0 < 0 or col0 + n_oicr * ncls > lin_weak.shape[1]:
        raise ValueError("similarity_ex: the refinement logit columns leave the row")
    sim = torch.empty((r, nn_, nb), dtype=torch.float32, device=lin_weak.device)
    check(lib().unit_similarity_ex(_p(lin_weak), lin_weak.shape[1], col0, n_oicr, ncls, _p(base_dev), nb, _p(a), nn_,
                                   *_plan_words(plan, visual_threshold), _p(sim), r, _s()), "similarity_ex")
    return sim


def similarity_bwd_ex(lin_weak, col0, n_oicr, ncls, base_dev, a, visual_threshold, plan, dsim, grad_dtype):
    """backward of `similarity_ex` -> d(loss)/d(lin_weak) [R, ld] (zeros for a plan without a per-RoI term)"""
    r, ld = lin_weak.shape
    nn_, nb = a.shape
    if tuple(dsim.shape) != (r, nn_, nb) or dsim.dtype != torch.float32:
        raise ValueError("similarity_bwd_ex: dsim must be fp32 [R, n_novel, n_base]")
    dlin = torch.empty((r, ld), dtype=grad_dtype, device=lin_weak.device)
    check(lib().unit_similarity_bwd_ex(_p(lin_weak), ld, col0, n_oicr, ncls, _p(base_dev), nb, _p(a), nn_, *_plan_words(plan, visual_threshold),
                                       _p(dsim), _p(dlin), dt(grad_dtype), ld, col0, r, _s()), "similarity_bwd_ex")
    return dlin


def softmax_rows(x, ncls):
    y = torch.empty((x.shape[0], ncls), dtype=torch.float32, device=x.device)
    check(lib().unit_softmax_rows(_p(x), x.shape[1], ncls, _p(y), ncls, x.shape[0], _s()), "softmax_rows")
    return y


def tta_accumulate(scores, deltas, k, r, v, n, probs_sum, delta_sum, delta_mean, count=None, n_in=1, view_rows=None, scol0=0):
    """adds the predictions of views v .. v + n_in - 1 of n (scores [.., ld] with K+1 columns from scol0, deltas [.., 4K]; R rows per view, the
    second view `view_rows` rows behind the first) to probs_sum [R,K+1] / delta_sum [R,4K] in view order; the last view writes delta_mean =
    delta_sum / n (unit_tta_accumulate: meta_arch/rcnn.py:516, :524)"""
    check(lib().unit_tta_accumulate(_p(scores), scores.shape[1], scol0, _p(deltas), deltas.shape[1], r if view_rows is None else int(view_rows),
                                    n_in, k, r, _p(count), v, n, _p(probs_sum), _p(delta_sum), _p(delta_mean), _s()), "tta_accumulate")


def max_detection_candidates():
    """the largest cand_cap the full form of `detections` takes: unit_nms's limit (the candidate kernel takes any cap, the sorter 2^20 keys)"""
    return int(lib().unit_nms_max_candidates())


def max_segmented_candidates():
    """the largest cand_cap the class-segmented form of `detections` takes (unit_detection_max_candidates: the sorter's 2^20 keys); on top of
    it a class holds at most max_detection_candidates() candidates, that is Rcap <= 65536"""
    return int(lib().unit_detection_max_candidates())


def detection_candidates(probs, deltas, props, pcount, image_hw, weights, score_thresh, cap):
    """the first stages of `detections`: unit_detection_candidates and the stable score sort -> (boxes [B,cap,4] clipped, scores [B,cap],
    classes int32 [B,cap], RoI rows int32 [B,cap] in (RoI, class) order, count int32 [B], max coordinate fp32 [B], order int32 [B,cap]: the
    candidate at each position of the descending score order, defined up to count[b])"""
    b, rcap = props.shape[0], props.shape[1]
    k = deltas.shape[1] // 4
    dev = probs.device
    cb = torch.empty((b, cap, 4), dtype=torch.float32, device=dev)
    cs = zeros((b, cap), torch.float32, dev)
    cc = torch.empty((b, cap), dtype=torch.int32, device=dev)
    cr = torch.empty((b, cap), dtype=torch.int32, device=dev)
    cnt = torch.empty((b,), dtype=torch.int32, device=dev)
    cmax = torch.empty((b,), dtype=torch.float32, device=dev)
    w = (ctypes.c_float * 4)(*weights)
    check(lib().unit_detection_candidates(_p(probs), probs.shape[1], _p(deltas), deltas.shape[1], _p(props), _p(pcount), b, rcap, k, w,
                                          SCALE_CLAMP, _p(image_hw), float(score_thresh), cap, _p(cb), _p(cs), _p(cc), _p(cr), _p(cnt),
                                          _p(cmax), _s()), "detection_candidates")
    # stable descending sort of the candidate scores (unused tail slots hold 0 <= thresh and sort behind every candidate)
    # (chip-wide select + rank sort over the valid candidates only: every valid score is > score_thresh >= 0 = the fill value)
    _, order = sort_desc(cs, b, cap, topk=cap, min_exclusive=0.0 if score_thresh >= 0 else None)
    return cb, cs, cc, cr, cnt, cmax, order


def detection_class_segments(cb, cs, cc, order, cnt, cmax, k, rseg):
    """the score-sorted candidates regrouped by class (unit_detection_class_segments) -> (seg_boxes [B*K,Rseg,4] shifted, seg_scores [B*K,Rseg],
    seg_count int32 [B*K], seg_pos int32 [B*K,Rseg]: the slot's position in its image's score order); slots behind seg_count are unwritten"""
    b, cap = cs.shape
    dev = cs.device
    sb = torch.empty((b * k, rseg, 4), dtype=torch.float32, device=dev)
    ss = torch.empty((b * k, rseg), dtype=torch.float32, device=dev)
    sp = torch.empty((b * k, rseg), dtype=torch.int32, device=dev)
    sn = torch.empty((b * k,), dtype=torch.int32, device=dev)
    nb = lib().unit_detection_segments_workspace_bytes(b, cap, k)
    ws = workspace(nb, dev)
    check(lib().unit_detection_class_segments(_p(cb), _p(cs), _p(cc), _p(order), _p(cnt), _p(cmax), b, cap, k, rseg, _p(sb), _p(ss), _p(sn),
                                              _p(sp), _p(ws), ws.numel(), _s()), "detection_class_segments")
    return sb, ss, sn, sp


def detection_merge_keep(seg_keep, seg_kc, seg_pos, b, k, cap):
    """the K per-class keep lists of every image merged by global position (unit_detection_merge_keep) -> (keep [B,topk] indices into the
    global score order, -1 behind the kept prefix; keep_count int32 [B])"""
    topk, rseg = seg_keep.shape[1], seg_pos.shape[1]
    dev = seg_keep.device
    kpos = torch.empty((b * k, topk), dtype=torch.int32, device=dev)
    keep = torch.empty((b, topk), dtype=torch.int32, device=dev)
    kc = torch.empty((b,), dtype=torch.int32, device=dev)
    check(lib().unit_detection_merge_keep(_p(seg_keep), _p(seg_kc), _p(seg_pos), b, k, rseg, cap, topk, _p(kpos), _p(keep), _p(kc), _s()),
          "detection_merge_keep")
    return keep, kc


def segmented_nms(cb, cs, cc, order, cnt, cmax, k, rseg, nms_thresh, topk, want_parts=False):
    """the NMS stage of `detections` in its class-segmented form: class segments -> unit_nms on the B * K segments (max_keep = topk, exact: a
    class cannot put more than topk boxes into the global top topk) -> merge. -> (keep [B,topk], keep_count [B]) as `nms` returns them.
    want_parts: additionally (seg_count, seg_pos, seg_keep, seg_keep_count), for the tests"""
    b, cap = cs.shape
    dev = cs.device
    sb, ss, sn, sp = detection_class_segments(cb, cs, cc, order, cnt, cmax, k, rseg)
    skeep = torch.empty((b * k, topk), dtype=torch.int32, device=dev)          # unit_nms writes the tails (-1) itself
    skc = torch.empty((b * k,), dtype=torch.int32, device=dev)
    nb = lib().unit_nms_workspace_bytes(b * k, rseg)
    ws = workspace(nb, dev)
    with _timed("nms_segmented", 0.0, b * cap * 20.0):
        check(lib().unit_nms(_p(sb), _p(ss), _p(sn), b * k, rseg, float(nms_thresh), topk, _p(skeep), _p(skc), None, None, _p(ws), ws.numel(),
                             _s()), "nms")
    keep, kc = detection_merge_keep(skeep, skc, sp, b, k, cap)
    return (keep, kc, (sn, sp, skeep, skc)) if want_parts else (keep, kc)


_full_nms = nms          # (`detections` has a keyword of that name)


def detections(probs, deltas, props, pcount, image_hw, weights, score_thresh, nms_thresh, topk, cand_cap=None, nms=None):
    """fast_rcnn_inference for B images: probs [B*Rcap, K+1], deltas [B*Rcap, 4K], props [B,Rcap,4], pcount [B] (device)
    -> (boxes [B,topk,4], scores [B,topk], classes [B,topk], roi_idx [B,topk], count [B]); rows past count[b] hold 0 / 0 / -1 / -1.
    Non-finite predictions: a RoI is dropped WHOLE when any of its K decoded boxes (before clipping; a NaN dw / dh is not clamped away)
    or any of its K+1 scores, background included, is non-finite -- detectron2's row filter in fast_rcnn_inference_single_image.
    roi_idx counts the image's ORIGINAL proposal rows (gather_rows on similarity['seg'] needs those); the reference reports indices into
    its filtered rows, which differ once a row was dropped.
    Ties in score keep (RoI, class) order (stable sort). More than `cand_cap` candidates above the threshold (default min(Rcap * K,
    65536)): the first cand_cap in (RoI, class) order go on to the sort and NMS, the rest are cut silently, whatever their scores.
    nms: the form of the NMS stage. "full": one all-pairs problem over the class-shifted list (unit_nms; cand_cap <=
    max_detection_candidates() = 65536, workspace quadratic in cand_cap). "segmented": one problem per (image, class) of at most Rcap boxes
    and a merge by score order (cand_cap <= max_segmented_candidates(), Rcap <= 65536; refused before anything launches otherwise). Both give
    the same result bit for bit. None: "full" where it fits, "segmented" above it -- a caller may pass a cand_cap up to Rcap * K beyond 65536."""
    b, rcap = props.shape[0], props.shape[1]
    k = deltas.shape[1] // 4
    dev = probs.device
    cap = cand_cap or min(rcap * k, 65536)
    if nms not in (None, "full", "segmented"):
        raise ValueError("detections: nms must be None, 'full' or 'segmented'")
    segmented = nms == "segmented" or (nms is None and cap > max_detection_candidates())
    rseg = max(min(rcap, cap), 1)          # a RoI contributes at most one candidate per class
    if segmented:
        check(lib().unit_detection_segments_check(b, cap, k, rseg), "detection_class_segments")
    cb, cs, cc, cr, cnt, cmax, order = detection_candidates(probs, deltas, props, pcount, image_hw, weights, score_thresh, cap)
    if segmented:
        keep, kc = segmented_nms(cb, cs, cc, order, cnt, cmax, k, rseg, nms_thresh, topk)
    else:
        ob = torch.empty((b, cap, 4), dtype=torch.float32, device=dev)
        check(lib().unit_detection_offset_gather(_p(cb), _p(cc), _p(order), _p(cnt), _p(cmax), b, cap, _p(ob), _s()), "detection_offset_gather")
        keep, kc, _, _ = _full_nms(ob, cs, cnt, nms_thresh, topk)
    oboxes = torch.empty((b, topk, 4), dtype=torch.float32, device=dev)
    oscores = torch.empty((b, topk), dtype=torch.float32, device=dev)
    ocls = torch.empty((b, topk), dtype=torch.int32, device=dev)
    oroi = torch.empty((b, topk), dtype=torch.int32, device=dev)
    ocnt = torch.empty((b,), dtype=torch.int32, device=dev)
    check(lib().unit_detection_finalize(_p(cb), _p(cs), _p(cc), _p(cr), _p(order), _p(keep), _p(kc), b, cap, topk, _p(oboxes), _p(oscores),
                                        _p(ocls), _p(oroi), _p(ocnt), _s()), "detection_finalize")
    return oboxes, oscores, ocls, oroi, ocnt


def detector_postprocess(boxes, count, scale_xy, out_hw):
    b, topk = boxes.shape[0], boxes.shape[1]
    nonempty = torch.empty((b, topk), dtype=torch.uint8, device=boxes.device)
    check(lib().unit_detector_postprocess(_p(boxes), _p(count), b, topk, _p(scale_xy), _p(out_hw), _p(nonempty), _s()), "detector_postprocess")
    return nonempty


def compact_detections(boxes, sc, cls, roi, cnt, nonempty=None, masks=None):
    """stable compaction of each image's kept detections (j < cnt[b] and nonempty[b][j]) to the front of its block (unit_compact_detections)
    -> (boxes, scores, classes int64, roi index, masks | None, kept count int32 [B])"""
    b, topk = boxes.shape[0], boxes.shape[1]
    dev = boxes.device
    ob, osc = torch.empty_like(boxes), torch.empty_like(sc)
    ocls = torch.empty((b, topk), dtype=torch.int64, device=dev)
    oroi = torch.empty_like(roi)
    om = torch.empty_like(masks) if masks is not None else None
    kept = torch.empty((b,), dtype=torch.int32, device=dev)
    me = masks[0, 0].numel() if masks is not None else 0
    check(lib().unit_compact_detections(_p(boxes), _p(sc), _p(cls), _p(roi), _p(masks), me, _p(cnt), _p(nonempty), b, topk, _p(ob), _p(osc), _p(ocls),
                                        _p(oroi), _p(om), _p(kept), _s()), "compact_detections")
    return ob, osc, ocls, oroi, om, kept


def pseudo_gt(boxes, scores, classes, count, multihot, threshold):
    """rcnn.py:594-599 (unit_pseudo_gt): detections boxes [N,T,4] / scores [N,T] / classes int32 [N,T] / count int32 [N] of the weak images,
    multihot uint8 [N,K] -> (gt_boxes [N,T,4]: the rows whose class is a label of the image and whose score is > threshold, at the front in
    detection order, zeros behind; gt_count int32 [N]; kept_idx int32 [N,T]: their row numbers, -1 behind). Everything stays on the device."""
    n, t = scores.shape
    assert classes.dtype == torch.int32 and count.dtype == torch.int32 and multihot.dtype == torch.uint8 and multihot.shape[0] == n
    assert boxes.is_contiguous() and scores.is_contiguous() and classes.is_contiguous() and multihot.is_contiguous()
    dev = boxes.device
    gt_boxes = torch.empty((n, t, 4), dtype=torch.float32, device=dev)
    gt_count = torch.empty((n,), dtype=torch.int32, device=dev)
    kept = torch.empty((n, t), dtype=torch.int32, device=dev)
    check(lib().unit_pseudo_gt(_p(boxes), _p(scores), _p(classes), _p(count), _p(multihot), n, t, multihot.shape[1], float(threshold),
                               _p(gt_boxes), _p(gt_count), _p(kept), _s()), "pseudo_gt")
    return gt_boxes, gt_count, kept


def gate_anchor_labels(labels, gt_count):
    """in place: the int8 anchor labels [N,Ncap] of every image with gt_count <= 0 become -1 (rcnn.py:607-609: such an image adds 0)"""
    assert labels.dtype == torch.int8 and labels.is_contiguous() and gt_count.dtype == torch.int32
    check(lib().unit_gate_anchor_labels(_p(labels), _p(gt_count), labels.shape[0], labels.shape[1], _s()), "gate_anchor_labels")
    return labels


def boxes_to_rois5(boxes):
    """[B,T,4] -> [B*T,5] RoIAlign rows (image index, box)"""
    b, t = boxes.shape[0], boxes.shape[1]
    out = torch.empty((b * t, 5), dtype=torch.float32, device=boxes.device)
    check(lib().unit_boxes_to_rois5(_p(boxes), b, t, _p(out), _s()), "boxes_to_rois5")
    return out


def gather_rows(src, idx, rcap):
    """src [B*rcap, ...] rows, idx int32 [B,T] (negative = row 0) -> [B*T, ...] = src[b*rcap + idx[b][j]]"""
    b, t = idx.shape
    row = src[0].numel() * src.element_size()
    out = torch.empty((b * t,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    check(lib().unit_gather_rows(_p(src), _p(idx), b, t, rcap, row, _p(out), _s()), "gather_rows")
    return out


def gather_blocks(src, nb, block_rows, take):
    """src [nb*block_rows, ...] (or more rows) -> dense [nb*take, ...]: the first `take` rows of every block (one launch instead of a
    torch.cat of nb slices)"""
    assert src.is_contiguous() and src.shape[0] >= nb * block_rows
    x3 = type(src) is X3
    row = src[0].numel() * src.element_size()
    out = torch.empty((nb * take,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if x3:
        out = out.as_subclass(X3)
    ptr = (lambda t: ctypes.c_void_p(t.data_ptr())) if x3 else _p
    check(lib().unit_gather_blocks(ptr(src), nb, block_rows, take, row, ptr(out), _s()), "gather_blocks")
    return out


def paste_masks(probs, boxes, out_hw, threshold=0.5, valid=None):
    """probs [S,M,M] fp32, boxes [S,4] (output-image coordinates) -> uint8 [S,H,W]  (detector_postprocess mask pasting)"""
    s, m = probs.shape[0], probs.shape[-1]
    h, w = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((s, h, w), dtype=torch.uint8, device=probs.device)
    check(lib().unit_paste_masks(_p(probs.contiguous()), _p(boxes.contiguous()), _p(valid), s, m, h, w, float(threshold), _p(out), _s()),
          "paste_masks")
    return out


def sum_losses(losses, out=None):
    out = out if out is not None else torch.empty(1, dtype=torch.float32, device=losses.device)
    check(lib().unit_sum_losses(_p(losses), losses.numel(), _p(out), _s()), "sum_losses")
    return out


def sgd_momentum(p, g, buf, lr, momentum, weight_decay, grad_scale=1.0, first_step=False, lr_dev=None):
    check(lib().unit_sgd_momentum(_p(p), _p(g), _p(buf), p.numel(), float(lr), float(momentum), float(weight_decay), float(grad_scale),
                                  int(first_step), _p(lr_dev), _s()), "sgd_momentum")


# ------------------------------------------------------------------------------------------------ gradient clipping + Nesterov (csrc/optim.hip)
CLIP_CHUNK = 16384          # elements per chunk of unit_grad_clip_coefs (unit_grad_clip_chunk(): checked by grad_clip_workspace)
NORM_KINDS = {float("inf"): 0, 1.0: 1, 2.0: 2}          # NORM_TYPE -> norm_kind
CLIP_NONE, CLIP_VALUE, CLIP_COEF = 0, 1, 2          # unit_sgd_step clip_mode


def clip_chunks(numel):
    """how many chunks unit_grad_clip_coefs cuts a tensor of `numel` elements into"""
    return (int(numel) + CLIP_CHUNK - 1) // CLIP_CHUNK


def grad_clip_workspace(g_numel, n_seg, device):
    """the caller-owned scratch of grad_clip_coefs for a gradient buffer of g_numel elements and a table of n_seg rows"""
    assert lib().unit_grad_clip_chunk() == CLIP_CHUNK
    return torch.empty(lib().unit_grad_clip_workspace_bytes(int(g_numel), int(n_seg)) // 8, dtype=torch.float64, device=device)


def grad_clip_coefs(g, table, seg_lo, seg_hi, n_chunks, norm_type, clip_value, grad_scale, norms, coefs, workspace, full_model=False):
    """norms[r] = ||g[table[r, 0] : + table[r, 1]] * grad_scale||_p and coefs[r] = min(1, clip_value / (norms[r] + 1e-6)) for the rows
    seg_lo <= r < seg_hi of `table` (int64 [n_seg, 2] on the device: offset, numel; ascending, disjoint); full_model: one coefficient
    from the norm over all rows of the range. n_chunks = sum(clip_chunks(numel)) over the range (the caller knows its table on the host;
    a wrong count makes the range NaN). Two launches, bit-identical from run to run, nothing allocated."""
    assert g.dtype == torch.float32 and g.is_contiguous() and table.dtype == torch.int64 and table.is_contiguous() and table.dim() == 2
    assert norms.dtype == torch.float32 and coefs.dtype == torch.float32 and norms.numel() >= table.shape[0] and coefs.numel() >= table.shape[0]
    assert norms.is_contiguous() and coefs.is_contiguous() and workspace.is_contiguous()
    check(lib().unit_grad_clip_coefs(_p(g), g.numel(), _p(table), table.shape[0], int(seg_lo), int(seg_hi), int(n_chunks),
                                     NORM_KINDS[float(norm_type)], float(clip_value), float(grad_scale), int(bool(full_model)), _p(norms), _p(coefs),
                                     _p(workspace), workspace.numel() * workspace.element_size(), _s()), "grad_clip_coefs")


def sgd_step(p, g, buf, lo, n, lr, momentum, weight_decay, grad_scale=1.0, first_step=False, lr_dev=None, nesterov=False,
             clip_mode=CLIP_NONE, clip_value=0.0, table=None, coefs=None):
    """sgd_momentum on the range [lo, lo + n) of the flat buffers p / g / buf, with gs = clip(g * grad_scale) (CLIP_VALUE: clamp to
    +-clip_value; CLIP_COEF: times coefs[row of the element in `table`], 1 outside every row) and torch's Nesterov form. g is not written."""
    assert p.dtype == g.dtype == buf.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous() and buf.is_contiguous()
    assert 0 <= lo and lo + n <= min(p.numel(), g.numel(), buf.numel())
    if clip_mode == CLIP_COEF:
        assert table.dtype == torch.int64 and table.is_contiguous() and coefs.dtype == torch.float32 and coefs.numel() >= table.shape[0]
    check(lib().unit_sgd_step(_p(p), _p(g), _p(buf), int(lo), int(n), float(lr), float(momentum), float(weight_decay), float(grad_scale),
                              float(clip_value), int(first_step), int(bool(nesterov)), int(clip_mode), _p(table),
                              0 if table is None else table.shape[0], _p(coefs), _p(lr_dev), _s()), "sgd_step")


def sgd_step_masked(p, g, buf, lo, n, lr, momentum, weight_decay, table, live, grad_scale=1.0, first_step=False, lr_dev=None, nesterov=False,
                    clip_mode=CLIP_NONE, clip_value=0.0, coefs=None):
    """sgd_step that leaves the tensors of dead rows untouched: `live` uint8 [table rows] on the device, 0 = p and buf of that row keep
    their bits whatever g holds (torch.optim.SGD on a parameter whose .grad is None). Live rows and padding: sgd_step's result bit for bit.
    The table is needed in every clip_mode."""
    assert p.dtype == g.dtype == buf.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous() and buf.is_contiguous()
    assert 0 <= lo and lo + n <= min(p.numel(), g.numel(), buf.numel())
    assert table is not None and table.dtype == torch.int64 and table.is_contiguous() and table.dim() == 2
    if live is not None:
        assert live.dtype == torch.uint8 and live.is_contiguous()
        if live.numel() != table.shape[0]:
            raise ValueError(f"sgd_step_masked: {live.numel()} live flags for a table of {table.shape[0]} rows")
    if clip_mode == CLIP_COEF:
        assert coefs.dtype == torch.float32 and coefs.numel() >= table.shape[0]
    check(lib().unit_sgd_step_masked(_p(p), _p(g), _p(buf), int(lo), int(n), float(lr), float(momentum), float(weight_decay), float(grad_scale),
                                     float(clip_value), int(first_step), int(bool(nesterov)), int(clip_mode), _p(table), table.shape[0],
                                     _p(coefs), _p(live), _p(lr_dev), _s()), "sgd_step_masked")


# ------------------------------------------------------------------------------------------------ training metrics (csrc/metrics.hip)
def metrics_rpn(labels, m):
    """m[0] += #(label == 1), m[1] += #(label == 0) over the sampled anchor labels (int8, any shape); m: int32 counters, zeroed by the caller"""
    assert labels.dtype == torch.int8 and labels.is_contiguous() and m.dtype == torch.int32 and m.numel() >= 2
    check(lib().unit_metrics_rpn(_p(labels), labels.numel(), _p(m), _s()), "metrics_rpn")


def metrics_fastrcnn(scores, col0, ncls, roi_cls, m):
    """the counts behind fast_rcnn/* and roi_head/* of one classifier batch: scores fp32 [R, ld] (columns col0 .. col0 + ncls, background last),
    roi_cls int32 [R] (outside [0, ncls - 1]: empty slot) -> m[0..5) += instances, correct, foreground, foreground correct, foreground called
    background"""
    r, ld = scores.shape
    assert scores.dtype == torch.float32 and scores.stride(1) == 1 and roi_cls.dtype == torch.int32 and roi_cls.numel() == r
    assert m.dtype == torch.int32 and m.numel() >= 5
    check(lib().unit_metrics_fastrcnn(_p(scores), scores.stride(0) if r > 1 else ld, col0, ncls, _p(roi_cls), r, _p(m), _s()), "metrics_fastrcnn")


def metrics_mask(logits, k, ldk, cls, targets, m):
    """the counts behind mask_rcnn/*: logits / cls / targets as unit_mask_bce_loss takes them (targets uint8 [S, M, M]) -> m[0..5) += elements,
    wrong, positives, false positives, false negatives"""
    s, msz = targets.shape[0], targets.shape[-1]
    assert logits.dtype == torch.float32 and cls.dtype == torch.int32 and targets.dtype == torch.uint8 and m.dtype == torch.int32 and m.numel() >= 5
    check(lib().unit_metrics_mask(_p(logits), k, ldk, _p(cls), _p(targets), s, msz, _p(m), _s()), "metrics_mask")
