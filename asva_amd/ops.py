"""Torch-tensor front end of the C ABI (include/avsd.h): one thin function per entry point.

Tensors are device-resident; activations are channels-last bf16 matrices [rows, C].  Every call
launches on torch's current HIP stream, so a `torch.cuda.graph` capture records the whole step.
PyTorch is used for memory and streams only; all arithmetic happens in libavsd_hip.so.
"""
from __future__ import annotations

import os
import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from . import precision as P
from ._lib import GemmDesc, XAttnDesc, check

PLAIN, TMIX, CONV3 = 0, 1, 2
GEGLU, OUT_F32, GELU, XCD_N, ROWSTATS, LNFUSE, RES1_F32, RES2_F32, X2, KROT, W_FRAG, OUT_REST = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048
_XCD_MODE = "auto"     # auto | m | n  (which operand each XCD's L2 fetches once)
F32 = torch.float32      # (16-bit storage dtype: P.ACT, asva_amd/precision.py)


class KernelTimer:
    """Optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg): while
    installed via `set_timer`, every wrapper below brackets its launch with two events and records
    (family, algorithmic flops, algorithmic bytes).  Off (None) in the product path."""

    def __init__(self):
        self.records = []
        self.replays = []      # (family, callable re-issuing the identical launch, tensors kept alive)

    def start(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def stop(self, ev0, family: str, flops: float, nbytes: float, flops_once: Optional[float] = None, flops_ref: Optional[float] = None):
        """flops: multiply-adds x 2 the launch ISSUES (the three passes of a split product counted three times); flops_once: the same
        product at one pass; flops_ref: the product as the reference states it (one pass; the 3x3 taps on the upsampled image for the
        sub-pixel form of the upsample convolution)"""
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        once = flops if flops_once is None else flops_once
        self.records.append((family, flops, nbytes, ev0, ev1, once, once if flops_ref is None else flops_ref))

    def add_replay(self, family: str, fn, keep):
        self.replays.append((family, fn, keep))

    def replay_ms(self, families, reps: int = 3) -> float:
        """GPU time of all recorded launches of `families`, issued back to back from one captured graph (no per-launch
        event, no host launch floor): what a rocprofv3 kernel trace of the graph-replayed step sees for them."""
        fns = [fn for fam, fn, _ in self.replays if fam in families]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for fn in fns:
                fn()
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for fam, fl, nb, e0, e1, fo, fr in self.records:
            d = out.setdefault(fam, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "flops_once": 0.0, "flops_ref": 0.0})
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += nb
            d["flops_once"] += fo
            d["flops_ref"] += fr
        return out


_TIMER: Optional[KernelTimer] = None


def set_timer(t: Optional[KernelTimer]) -> None:
    global _TIMER
    _TIMER = t


def _timed(family: str, flops: float, nbytes: float, keep, *calls) -> None:
    """issues `calls` (zero-argument callables, one library launch each, reading the current stream when called) and, under a
    KernelTimer, records their event-pair time and registers them for the graph-replayed per-family timing"""
    ev = _TIMER.start() if _TIMER is not None else None
    for c in calls:
        c()
    if ev is not None:
        _TIMER.add_replay(family, lambda: [c() for c in calls], keep)
        _TIMER.stop(ev, family, flops, nbytes)


def _nbytes(*ts) -> float:
    return float(sum(t.numel() * t.element_size() for t in ts if t is not None))


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---- per-shape tile selection ---------------------------------------------------------------------------
# The GEMM kernel exists in several tile/wave/stage configurations (gemm.hip: dispatch_tile).  Which one is
# fastest depends on (mode, M, N, K, epilogue).  Selection is DETERMINISTIC by default, so two processes produce
# bit-identical results (the f32 summation order depends on the tile):
#   1. the committed table asva_amd/tiles_gfx950.json (tuned on MI355X for the BASELINE.json shapes by
#      tools/tune_tiles.py; AVSD_TILE_CACHE=<file> replaces it),
#   2. else a static rule of thumb (_heuristic_tile): the largest tile that still yields >= ~1 workgroup per CU, split-K
#      for the low-resolution layers.
# AVSD_AUTOTUNE=1 / set_autotune(True) switches on the measuring tuner for shapes missing from the table: every
# candidate is timed with HIP events on the caller's real buffers and the winner is cached for the life of the
# process (measure, don't guess) — that is how the table is produced; results then depend on timing noise.
TILE_CANDIDATES = ((4, 1), (6, 1), (7, 1), (9, 1), (3, 1), (11, 1), (12, 1), (13, 1), (14, 1), (17, 1), (19, 1),
                   (20, 1), (24, 1), (25, 1), (30, 1), (31, 1), (38, 1))
# extra (tile, split_k) candidates for GEMMs whose output is too small to fill 256 CUs with big tiles
SPLITK_CANDIDATES = ((6, 2), (6, 4), (6, 8), (9, 2), (9, 4), (4, 2), (4, 4), (4, 8), (7, 2), (7, 4),
                     (20, 2), (20, 4), (24, 2), (24, 4), (24, 8), (25, 2), (25, 4),
                     (30, 2), (30, 4), (30, 8), (31, 2), (31, 4), (31, 8))
# split precision (AVSD_GEMM_X2): the tiles whose doubled LDS stage fits (gemm.hip dispatch_tile_x2)
X2_TILE_CANDIDATES = ((7, 1), (11, 1), (13, 1), (24, 1), (25, 1), (34, 1), (35, 1), (36, 1))
X2_SPLITK_CANDIDATES = ((34, 2), (34, 4), (35, 2), (35, 4), (36, 2), (36, 4), (7, 2), (7, 4), (7, 8), (11, 2), (11, 4), (24, 2), (24, 4), (24, 8), (25, 2), (25, 4), (25, 8))
# 3x3 stride-1 convolutions with the input tile resident in LDS (csrc/conv3r.hip): tile ids 40-49, geometry-dependent
# (avsd_gemm_conv3r_supported); split_k cuts the cin / 64 channel chunks
# 4-wave tiles with a hand-scheduled main loop (csrc/gemm4.hip): 60 = 256x256, 61 = 256x128, 62 = 128x256, 63 = 128x128; PLAIN, K % 64 == 0
# 64 = 128x64, 65 = 64x128, 66 = 64x64, 67 = 128x320 (the N = 320 layers in one column tile); TMIX (cseg % 64 == 0): 61..67
ASM_CANDIDATES = ((60, 1), (61, 1), (62, 1), (63, 1), (64, 1), (65, 1), (66, 1), (67, 1))
ASM_SPLITK_CANDIDATES = ((63, 2), (63, 4), (63, 8), (61, 2), (62, 2), (62, 4), (64, 2), (64, 4), (65, 2), (65, 4), (66, 2), (66, 4),
                         (67, 2), (67, 3), (67, 4), (67, 5), (67, 6))
ASM_TILES = tuple(range(60, 68))
# column-tile width of the LDS-direct tile ids (gemm.hip dispatch_tile / dispatch_tile_x2): a sub-pixel upsample convolution (ups = 2) needs
# whole column tiles per output-pixel parity, cout % BN == 0.  These constants, the candidate tuples above and what the two rules return
# are hand copies of the `switch` statements in csrc/gemm.hip: tests/test_tile_choice_cpu.py parses that file and pins them
SUBPIX_TILES = (4, 6, 9, 11, 13, 17, 20, 24, 25, 30, 38)          # gemm.hip avsd_gemm_dispatch_subpix / _x2_subpix
SUBPIX_X2_TILES = (7, 11, 13, 24, 25, 34, 35)
TILE_BN = {4: 64, 6: 128, 7: 64, 9: 128, 11: 128, 12: 64, 13: 64, 14: 128, 17: 320, 19: 320, 20: 128, 24: 64, 25: 64, 30: 128, 31: 256, 34: 160,
           35: 64, 36: 192, 38: 160}
# a pick the sub-pixel loader is not built for -> the built tile of the same block (the deeper ring / the loader-wave form), and the
# tile that stands for each column width when the pick has to narrow (128 x BN, the rule's own 128 x 128 / 128 x 64 picks)
_SUBPIX_RELATIVE = {14: 20, 12: 24, 19: 17, 7: 25}
_SUBPIX_BY_BN = ({320: 17, 160: 38, 128: 11, 64: 24}, {160: 34, 128: 11, 64: 24})
ASM_X2_CANDIDATES = ((63, 1), (64, 1), (65, 1), (66, 1))        # split precision: 128x128 ... 64x64
ASM_X2_SPLITK_CANDIDATES = ((63, 2), (63, 4), (64, 2), (64, 4), (65, 2), (65, 4), (66, 2), (66, 4), (66, 8))
_ASM_TILES = True          # (module attribute: tools set it to False to time the LDS-direct tiles alone)
# Row bands start their K walk at different tiles (AVSD_GEMM_KROT, include/avsd.h; LDS-direct, resident-convolution and asm tiles) — the
# weights of the low-resolution layers come from HBM inside a step, and a lockstep walk is one chain of round trips.
# AVSD_KROT=0 / set_krot(False): the unrotated walk (every tile of a family then sums K in the same order).
_KROT = os.environ.get("AVSD_KROT", "1") != "0"
_KROT_ASM_ONLY = False          # probe (profiles/r4_krot_ab.txt): rotate the asm tiles only
# ... and only where the weights one XCD walks (its share of W under the column banding) stay in its 4-MB L2 for a whole rotation: bands
# that stand at different K positions re-read W a rotation apart, so a larger W (the 3x3 convolutions at 8 x 8: 29 MB) would come from
# the Infinity Cache once per band instead of once (measured: rotating everything 80.9 steps/s, this rule 81.8, nothing 80.0)
_KROT_MAX_W = 16 << 20


def set_krot(on: bool) -> None:
    global _KROT
    _KROT = bool(on)


def _subpix_tile(tile: int, cout: int, x2: bool) -> int:
    """the tile a sub-pixel upsample convolution (ups = 2) runs on when the table or the rule named `tile`: `tile` itself if this loader
    builds it and its column tiles are whole per output-pixel parity (cout % BN == 0, gemm.hip launch2), else its built relative, else the
    widest built column tile that divides cout and is no wider than the pick.  cout % 64 == 0 (gemm()'s gate), so the 64-wide tiles make
    this total.  Every tile of the two sets is LDS-direct and splits K, so the caller's split_k stands whatever comes back."""
    if cout <= 0 or cout % 64:
        raise ValueError(f"gemm: ups = 2 needs cout % 64 == 0 (got {cout})")
    built = SUBPIX_X2_TILES if x2 else SUBPIX_TILES

    def ok(t):
        return t in built and cout % TILE_BN[t] == 0

    if ok(tile):
        return tile
    if ok(_SUBPIX_RELATIVE.get(tile, 0)):
        return _SUBPIX_RELATIVE[tile]
    bn0 = TILE_BN.get(tile, 128)          # (register-staged, resident and asm ids carry no width here: treated as the 128-wide default)
    return next(t for bn, t in sorted(_SUBPIX_BY_BN[int(x2)].items(), reverse=True) if bn <= max(bn0, 64) and ok(t))


# A-resident, N-streaming tile (csrc/nstream.hip): the wide short-K projections whose weights the caller also holds in fragment order.
# Chosen by rule, not by the table: it needs the second weight layout, which only the caller can provide (gemm(w_frag=...)).
NSTREAM_TILE = 70
_NSTREAM = os.environ.get("AVSD_NSTREAM", "1") != "0"


def nstream_supported(M: int, N: int, K: int) -> bool:
    """the shapes tile 70 is built for: all of A's K in LDS (K = 320 / 640), at least 8 N fragments per wave set, and N wide enough that
    streaming it pays (N >= 4 K: the GEGLU projections; a square layer is better off on the tiled kernels)"""
    return K in (320, 640) and N % 256 == 0 and N >= 4 * K and M >= 96


_RASTER_G = 0       # probe knob: rows of the tile blocks an XCD walks (0 = the kernel's default)
CONV3R_TILES = (40, 42, 43, 44, 48)
CONV3R2D_TILES = (51, 52, 53, 54)   # rectangular resident tiles (TH rows x 32 pixels) for images wider than 32 pixels: the VAE decoder, cfg 4
_CONV3R2D_BN = {51: 128, 52: 160, 53: 128, 54: 128}
CONV3R_SPLITS = (1, 2, 4, 5, 8, 10)
_CONV3R = True


_CONV3R_BN = (128, 128, 160, 160, 128, 128, 256, 320, 256, 64)


def conv3r_candidates(hs: int, ws: int, cin: int, M: int, N: int, one_d_only: bool = False):
    """(tile, split_k) pairs of the LDS-resident convolution tiles that fit this image geometry and leave >= 2 chunks per slice"""
    out = []
    for t in CONV3R_TILES:
        bm = _lib.lib().avsd_gemm_conv3r_supported(t, hs, ws, cin)
        if bm <= 0:
            continue
        bn = _CONV3R_BN[t - 40]
        wgs = ((M + bm - 1) // bm) * ((N + bn - 1) // bn)
        for sk in CONV3R_SPLITS:
            if sk > 1 and (wgs >= 256 or (cin // 64) // sk < 2 or (cin // 64) % sk != 0):
                continue
            out.append((t, sk))
    if not one_d_only:
        for t in CONV3R2D_TILES:
            bm = _lib.lib().avsd_gemm_conv3r2d_supported(t, hs, ws, cin)
            if bm <= 0:
                continue
            wgs = (M // bm) * ((N + _CONV3R2D_BN[t] - 1) // _CONV3R2D_BN[t])
            for sk in CONV3R_SPLITS:
                if sk > 1 and (wgs >= 256 or (cin // 64) // sk < 2 or (cin // 64) % sk != 0):
                    continue
                out.append((t, sk))
    return tuple(out)


def _heuristic_conv3r(cands, M: int, N: int):
    """static pick among the admissible resident tiles when the table has no entry: the candidate that wastes the fewest
    padded columns, then the one closest to one workgroup per CU"""
    def cost(c):
        t, sk = c
        bn = _CONV3R_BN[t - 40] if t < 50 else _CONV3R2D_BN[t]
        bm = 256 if t in (40, 41, 42, 43, 48, 51, 52, 53) else 128
        wg = ((M + bm - 1) // bm) * ((N + bn - 1) // bn) * sk
        pad = ((N + bn - 1) // bn) * bn / N
        return (round(pad, 2), abs(wg - 256) if wg < 256 else (wg - 256) // 4, sk)
    return min(cands, key=cost)


_TILE_CACHE: dict = {}
_AUTOTUNE = os.environ.get("AVSD_AUTOTUNE", "0") == "1"


def set_autotune(on: bool) -> None:
    global _AUTOTUNE
    _AUTOTUNE = bool(on)


def tile_cache() -> dict:
    return _TILE_CACHE


def save_tile_cache(path: str) -> None:
    """Writes the tuned (shape -> tile, split_k) table as JSON; AVSD_TILE_CACHE=<path> loads it at import, so a
    profiling run (rocprofv3 --pmc serialises every dispatch) can skip the tuning launches."""
    import json

    with open(path, "w") as f:
        json.dump([[list(k), list(v)] for k, v in _TILE_CACHE.items()], f)


def load_tile_cache(path: str) -> int:
    import json

    with open(path) as f:
        for k, v in json.load(f):
            _TILE_CACHE[tuple(k)] = tuple(v)
    return len(_TILE_CACHE)


DEFAULT_TILE_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tiles_gfx950.json")
if os.environ.get("AVSD_TILE_CACHE"):
    if os.path.isfile(os.environ["AVSD_TILE_CACHE"]):
        load_tile_cache(os.environ["AVSD_TILE_CACHE"])
elif os.path.isfile(DEFAULT_TILE_TABLE):
    load_tile_cache(DEFAULT_TILE_TABLE)


def _heuristic_tile(M: int, N: int, K: int, geglu: bool, splitk_ok: bool):
    """Static (tile, split_k) for shapes the table does not hold.  Per-tile efficiency grows with the tile (the
    global->LDS path delivers (BM + BN) / (BM * BN) bytes per MFMA flop), but a launch wants >= ~1 workgroup per CU."""
    def tiles(bm, bn):
        return ((M + bm - 1) // bm) * ((N + bn - 1) // bn)

    nk = (K + 63) // 64
    # measured (profiles/r2_probes.md, tools/tile_probe.py): 256x128 wins once it fills the chip — with loader waves and a
    # 3-deep ring for long K, the 2-stage form for short K; 256x256 only pays at K >= 4096 and is left to the tuned table;
    # N = 320 layers lose 17 % of a 128-wide tile to padding and take 128x64
    if N >= 512 and tiles(256, 128) >= 224:
        return (20 if nk >= 16 else 14), 1
    if N >= 512 and tiles(128, 128) >= 224:
        return (30 if nk >= 8 else 11), 1
    if tiles(128, 64) >= 224:
        return (24 if nk >= 16 else 12), 1
    t64 = tiles(64, 64)
    if t64 >= 160 or not splitk_ok or geglu or nk < 8:
        return (25 if nk >= 8 else 13), 1
    sk = 1
    while sk < 8 and t64 * sk < 224 and nk // (2 * sk) >= 4:
        sk *= 2
    return 25, sk


def _heuristic_tile_x2(M: int, N: int, K: int, geglu: bool, splitk_ok: bool):
    """the same rule over the split-precision tile set: 128x128 (2-stage), 128x64, 64x64, split-K for the small outputs"""
    def tiles(bm, bn):
        return ((M + bm - 1) // bm) * ((N + bn - 1) // bn)

    nk = (K + 63) // 64
    if N % 160 == 0 and N <= 640 and tiles(128, 160) >= 224:
        return 34, 1
    if N >= 128 and tiles(128, 128) >= 224:
        return 11, 1
    if tiles(128, 64) >= 224:
        return 24, 1
    t64 = tiles(64, 64)
    if t64 >= 160 or not splitk_ok or geglu or nk < 8:
        return (25 if nk >= 8 else 13), 1
    sk = 1
    while sk < 8 and t64 * sk < 224 and nk // (2 * sk) >= 4:
        sk *= 2
    return 25, sk


_TUNE_COLD = True
_FLUSH = None


def _evict_weights(warm):
    """Reproduce the cache state a launch meets inside a denoising step: every weight is streamed from HBM once per
    step (2.3 GB of them pass between two uses), while the activations were written by the previous kernel.  Write a
    buffer larger than L2 + Infinity Cache, then read the activations back in."""
    global _FLUSH
    if _FLUSH is None:
        _FLUSH = torch.empty(384 << 20, dtype=torch.uint8, device="cuda")
    _FLUSH.zero_()
    for t in warm:
        if t is not None:
            t.view(torch.int16 if t.element_size() == 2 else torch.int32).max()


def _time_hot(launch, cand, reps=8):
    """GPU time per launch of `reps` back-to-back launches replayed from a captured graph: eager launches through
    Python/ctypes cannot be issued faster than one per ~11 us, which would hide every difference between candidates
    for the many GEMMs of this UNet that run 10-20 us."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            launch(*cand)
    g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / (2 * reps)


def _time_cold(launch, cand, warm, reps=7):
    ms = []
    for _ in range(reps):
        _evict_weights(warm)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(*cand)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


_CHALLENGE = os.environ.get("AVSD_TUNE_CHALLENGE", "0") == "1"     # tools/tune_tiles.py --challenge: re-time table entries against new tiles
_CHALLENGE_TILES = tuple(int(v) for v in os.environ.get("AVSD_TUNE_CHALLENGE_TILES", "").split(",") if v)      # ... against these tile ids only
_CHALLENGED: set = set()
RECORD_KEYS = None
CHALLENGE_LOG: list = []


def _challenge(key, launch, challengers, warm):
    """the table's entry for `key` against `challengers` (new tile ids): replaced when one of them is >= 3 % faster hot (two
    interleaved rounds, best-of) and not slower against cold weights"""
    inc = _TILE_CACHE[key]
    _CHALLENGED.add(key)
    if _CHALLENGE_TILES:
        challengers = tuple(c for c in challengers if c[0] in _CHALLENGE_TILES)
        if not challengers:
            return
    times = {}
    for rnd in range(2):
        for cand in (inc,) + tuple(c for c in challengers if c != inc):
            if rnd == 0:
                launch(*cand)
            times[cand] = min(_time_hot(launch, cand), times.get(cand, float("inf")))
    best = min(times, key=times.get)
    if best != inc and times[best] < 0.97 * times[inc] and (warm is None or _time_cold(launch, best, warm) < _time_cold(launch, inc, warm)):
        CHALLENGE_LOG.append((key, inc, best, times[inc] * 1e3, times[best] * 1e3))
        _TILE_CACHE[key] = best


def _pick_tile(key, launch, candidates=TILE_CANDIDATES, warm=None, challengers=()):
    """-> (tile, split_k).  Two passes: every candidate is timed back to back on a hot L2 (two interleaved rounds,
    best-of: robust to clock ramp / noise); the four fastest are then re-timed launch by launch against cold weights
    and warm activations (`warm`: the activation tensors; median of 7) — the state a launch meets inside a denoising
    step — and the winner of that pass is cached.  AVSD_TUNE_COLD=0 keeps the first pass only."""
    t = _TILE_CACHE.get(key)
    if t is not None:
        if _CHALLENGE and challengers and key not in _CHALLENGED and _AUTOTUNE and _TIMER is None and not torch.cuda.is_current_stream_capturing():
            _challenge(key, launch, challengers, warm)
            return _TILE_CACHE[key]
        return t
    if not _AUTOTUNE or _TIMER is not None or torch.cuda.is_current_stream_capturing():
        return None
    candidates = tuple(candidates) + tuple(challengers)
    times = {}
    for rnd in range(2):
        for cand in candidates:
            if rnd == 0:
                launch(*cand)              # warm (also sets the kernel's LDS attribute)
            times[cand] = min(_time_hot(launch, cand), times.get(cand, float("inf")))
    ranked = sorted(times, key=times.get)
    best = ranked[0]
    if _TUNE_COLD and warm is not None and len(ranked) > 1:
        finalists = ranked[:4]
        cold = {c: _time_cold(launch, c, warm) for c in finalists}
        best = min(cold, key=cold.get)
    _TILE_CACHE[key] = best
    return best


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# ---- split-precision storage (asva_amd/precision.py): a 16-bit tensor is a view into the FIRST half of its storage, its rest
# plane lies at the same offset in the second half ------------------------------------------------------------------------
def alloc16(shape, device) -> torch.Tensor:
    """uninitialised 16-bit activation tensor; in split mode the main plane of a twin allocation"""
    if not P.SPLIT:
        return torch.empty(shape, dtype=P.ACT, device=device)
    n = 1
    for d in shape:
        n *= int(d)
    npad = (n + 7) // 8 * 8
    return torch.empty((2, npad), dtype=P.ACT, device=device)[0, :n].view(tuple(shape))


def _lo(t: Optional[torch.Tensor]) -> int:
    """element offset from `t` to its rest plane (0 outside split mode / for None)"""
    if t is None or not P.SPLIT:
        return 0
    if t.dtype != P.ACT:
        raise TypeError(f"split precision: expected a {P.ACT} tensor, got {t.dtype}")
    nb = t.untyped_storage().nbytes()
    last = sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
    if nb % 32 or (t.storage_offset() + last + 1) * 2 > nb // 2:
        raise ValueError("split precision: tensor is not a view into the first half of a twin allocation "
                         "(allocate with ops.alloc16 / ops.to_act / weights.to_act)")
    return nb // 4


def to_act(x: torch.Tensor) -> torch.Tensor:
    """any float device tensor -> the 16-bit storage type (one launch in split mode: main and rest planes)"""
    if not P.SPLIT:
        return x.to(P.ACT).contiguous()
    x = x.to(F32).contiguous()
    out = alloc16(tuple(x.shape), x.device)
    check(_lib.lib().avsd_split_f32(_p(x), _p(out), _lo(out), x.numel(), _stream()), "avsd_split_f32")
    return out


def from_act(t: torch.Tensor) -> torch.Tensor:
    """f32 values of a 16-bit activation (main + rest in split mode); for tests and host-side checks"""
    if not P.SPLIT:
        return t.float()
    half = _lo(t)
    return t.float() + torch.as_strided(t, t.shape, t.stride(), t.storage_offset() + half).float()


def alloc_planes(shape, device):
    """(main, rest): two 16-bit planes of one allocation, whatever the process-wide mode — operands of an explicit three-pass
    product (gemm(..., a_rest=, w_rest=)) under the per-layer precision plan (asva_amd/precision.py)"""
    n = 1
    for d in shape:
        n *= int(d)
    npad = (n + 7) // 8 * 8
    buf = torch.empty((2, npad), dtype=P.ACT, device=device)
    return buf[0, :n].view(tuple(shape)), buf[1, :n].view(tuple(shape))


def split_planes(x: torch.Tensor):
    """f32 device tensor -> (main, rest) 16-bit planes: main = round16(x), rest = round16(x - main) (one launch)"""
    x = x.contiguous()
    _req(x, F32, "x")
    main, rest = alloc_planes(tuple(x.shape), x.device)
    check(_lib.lib().avsd_split_f32(_p(x), _p(main), _rest_off(main, rest), x.numel(), _stream()), "avsd_split_f32")
    return main, rest


def _rest_off(main: torch.Tensor, rest: Optional[torch.Tensor]) -> int:
    """element offset from `main` to its explicit rest plane (same shape and strides)"""
    if rest is None:
        return 0
    if rest.dtype != main.dtype or rest.shape != main.shape or rest.stride() != main.stride():
        raise ValueError("rest plane must match its main plane in dtype, shape and strides")
    off = rest.data_ptr() - main.data_ptr()
    if off == 0 or off % 16:
        raise ValueError("rest plane must be a distinct tensor, a multiple of 8 elements away from its main plane")
    return off // 2


def _req(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a device tensor (libavsd_hip.so has no host path)")
    if t.dim() >= 1 and t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost dimension must be contiguous")


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.dim() == 2 else t.stride(-2)


def gemm(
    a: torch.Tensor,
    w: torch.Tensor,
    *,
    n: Optional[int] = None,
    k: Optional[int] = None,
    a2: Optional[torch.Tensor] = None,
    bias: Optional[torch.Tensor] = None,
    rowvec: Optional[torch.Tensor] = None,
    rows_per_vec: int = 0,
    res1: Optional[torch.Tensor] = None,
    res2: Optional[torch.Tensor] = None,
    alpha: float = 1.0,
    geglu: bool = False,
    gelu: bool = False,
    rowstats: Optional[torch.Tensor] = None,   # out: f32 [M, N/32, 2] (sum, sumsq) of the rounded outputs per 32 columns
    ln: Optional[tuple] = None,                # (stats [rows, K/32, 2] f32, colsum [N] f32, eps): LayerNorm(A) folded in
    stats_pos: Optional[tuple] = None,         # (pos [frames, N] f32, hw, frames): rowstats of out + pos[frame of the row]
    ln_pos: Optional[tuple] = None,            # (pos . W'^T [frames, N] f32, hw, frames) with ln: LayerNorm(A + pos[frame]) folded in
    out_f32: bool = False,
    out: Optional[torch.Tensor] = None,
    master: Optional[torch.Tensor] = None,     # out: f32 [M, N] un-rounded copy of the result (f32 residual stream)
    mode: int = PLAIN,
    tmix: Optional[tuple] = None,      # (hw, frames)
    conv: Optional[tuple] = None,      # (n_img, hs, ws, stride, ups[, pad])
    m: Optional[int] = None,
    tile: int = 0,
    split_k: int = 1,
    a_rest: Optional[torch.Tensor] = None,     # explicit rest planes of a / a2 / w: THIS product runs as three MFMA passes (AVSD_GEMM_X2)
    a2_rest: Optional[torch.Tensor] = None,    # whatever the process-wide mode (per-layer precision plan); f32 output and f32 residuals
    w_rest: Optional[torch.Tensor] = None,
    out_rest: Optional[torch.Tensor] = None,   # out: the rest plane round16(v - out) of a 16-bit output (AVSD_GEMM_OUT_REST; with w_rest: the second
                                               # output plane of the three-pass product) — what split_planes(master) would make in another launch
    w_frag: Optional[torch.Tensor] = None,     # the same weights in MFMA-fragment order (weights.pack_frag): lets the A-resident N-streaming
                                               # tile (70, csrc/nstream.hip) take the product where it applies (nstream_supported)
) -> torch.Tensor:
    """out = epilogue(alpha * A' . W^T); see avsd_gemm_bf16 in include/avsd.h."""
    _req(a, P.ACT, "a")
    _req(w, P.ACT, "w")
    planes = w_rest is not None
    if planes:
        if P.SPLIT:
            raise ValueError("gemm: explicit rest planes are for the non-split modes (split precision carries them implicitly)")
        if a_rest is None or (a2 is not None) != (a2_rest is not None) or rowstats is not None or ln is not None:
            raise ValueError("gemm: a three-pass product needs a_rest and w_rest (a2_rest with a2), no rowstats / LayerNorm fold")
        if out_f32 == (out_rest is not None) or (out_f32 and master is not None):
            raise ValueError("gemm: a three-pass product writes f32 (out_f32) or a (main, rest) pair of planes (out=, out_rest=; optional f32 master)")
        if any(r is not None and r.dtype != F32 for r in (res1, res2)):
            raise ValueError("gemm: a three-pass product reads f32 residuals")
    elif a_rest is not None or a2_rest is not None:
        raise ValueError("gemm: a_rest / a2_rest without w_rest")
    if out_rest is not None and (P.SPLIT or out_f32 or geglu or out is None):
        raise ValueError("gemm: out_rest goes with an explicit 16-bit `out` outside split precision (no GEGLU)")
    x2 = P.SPLIT or planes
    if x2 and mode == PLAIN and a2 is not None and a.shape[1] % 64 != 0:
        # the LDS-direct loader switches source buffers per 64-wide K tile and the register-staged tiles have no split form:
        # a concat split inside a K tile (tiny test networks: 160-channel skips) runs as two launches, the first leaving its
        # un-rounded f32 partial for the second's epilogue — the same sum
        if res1 is not None and res2 is not None:
            raise ValueError("gemm: split precision with an unaligned two-source A supports one residual")
        if gelu or geglu or rowstats is not None or ln is not None or stats_pos is not None or ln_pos is not None or (master is not None and not planes) or n is not None \
                or k is not None or m is not None or tile or split_k != 1:
            # (GELU would be applied to the second partial alone; the other options are not forwarded by this two-launch form)
            raise ValueError("gemm: split precision with an unaligned two-source A takes bias / rowvec / one residual / alpha only")
        k1 = a.shape[1]
        part = gemm(a, w[:, :k1], alpha=alpha, out_f32=True, a_rest=a_rest, w_rest=None if w_rest is None else w_rest[:, :k1])
        return gemm(a2, w[:, k1:], bias=bias, rowvec=rowvec, rows_per_vec=rows_per_vec, res1=part, res2=res1 if res1 is not None else res2,
                    alpha=alpha, out_f32=out_f32, out=out, out_rest=out_rest, master=master, a_rest=a2_rest, w_rest=None if w_rest is None else w_rest[:, k1:])
    d = GemmDesc()
    N = w.shape[0] if n is None else n
    lda = _ld(a)
    if mode == PLAIN:
        M = a.shape[0] if m is None else m
        K1 = a.shape[1]
        K = K1 + (a2.shape[1] if a2 is not None else 0)
        if a2 is not None:
            _req(a2, P.ACT, "a2")
            d.A2, d.lda2, d.k_split = _p(a2), _ld(a2), K1
        else:
            d.k_split = K
        if k is not None:
            K = k
    elif mode == TMIX:
        hw, frames = tmix
        M = a.shape[0]
        cseg = a.shape[1]
        K = 3 * cseg
        d.hw, d.frames, d.cseg = hw, frames, cseg
    elif mode == CONV3:
        n_img, hs, ws, stride, ups = conv[:5]
        pad = conv[5] if len(conv) > 5 else 1
        cin = a.shape[1]
        if a2 is not None:              # two-source input: only the LDS-resident tiles read it (conv3r.hip)
            _req(a2, P.ACT, "a2")
            d.A2, d.lda2, d.k_split = _p(a2), _ld(a2), cin
            cin += a2.shape[1]
        if ups == 2:
            # nearest-2x upsample + 3x3 convolution as four per-parity 2x2 convolutions on the original image (weights.subpixel_conv3x3):
            # GEMM rows = INPUT pixels, columns = (parity, cout), K = 4 taps x cin; the epilogue scatters row m = (n, y, x), column
            # (dy, dx, co) to output pixel (n, 2 y + dy, 2 x + dx) of the [n_img * 2 hs * 2 ws, cout] result
            if stride != 1 or pad != 1 or a2 is not None or N % 4 or w.shape[1] != 4 * cin or cin % 64 or (N // 4) % 64:
                raise ValueError("gemm: ups = 2 (sub-pixel upsample convolution) needs stride 1, pad 1, one source, w [4 cout, 4 cin], cin % 64 == 0, cout % 64 == 0")
            if geglu or gelu or rowstats is not None or ln is not None or res1 is not None or res2 is not None or rowvec is not None:
                raise ValueError("gemm: ups = 2 takes bias / master / out_rest only")
            ho, wo = hs, ws
            M = n_img * hs * ws
            K = 4 * cin
        else:
            hin, win = hs << ups, ws << ups
            ho, wo = (hin + 2 - 3) // stride + 1, (win + 2 - 3) // stride + 1
            M = n_img * ho * wo
            K = 9 * cin
        d.hs, d.ws, d.ho, d.wo, d.cin, d.stride, d.ups, d.pad = hs, ws, ho, wo, cin, stride, ups, pad
    else:
        raise ValueError(f"unknown gemm mode {mode}")
    n_out = N // 2 if geglu else N
    m_out = M
    if mode == CONV3 and d.ups == 2:
        m_out, n_out = 4 * M, N // 4
    if out is None:
        out = torch.empty((m_out, n_out), dtype=F32, device=a.device) if out_f32 else alloc16((m_out, n_out), a.device)
    else:
        _req(out, F32 if out_f32 else P.ACT, "out")
        if tuple(out.shape) != (m_out, n_out) and mode == CONV3 and d.ups == 2:
            raise ValueError(f"gemm: ups = 2 writes [{m_out}, {n_out}], got {tuple(out.shape)}")
    d.A, d.W, d.out = _p(a), _p(w), _p(out)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldw, d.ldc = lda, _ld(w), _ld(out)
    if bias is not None:
        _req(bias, F32, "bias")
        d.bias = _p(bias)
    if rowvec is not None:
        _req(rowvec, F32, "rowvec")
        d.rowvec, d.rows_per_vec, d.ldv = _p(rowvec), rows_per_vec, _ld(rowvec)
    d.flags = (GEGLU if geglu else 0) | (OUT_F32 if out_f32 else 0) | (GELU if gelu else 0)
    if res1 is not None:            # residuals: 16-bit, or f32 (the f32 residual stream)
        _req(res1, F32 if res1.dtype == F32 else P.ACT, "res1")
        d.res1, d.ldr1 = _p(res1), _ld(res1)
        d.flags |= RES1_F32 if res1.dtype == F32 else 0
    if res2 is not None:
        _req(res2, F32 if res2.dtype == F32 else P.ACT, "res2")
        d.res2, d.ldr2 = _p(res2), _ld(res2)
        d.flags |= RES2_F32 if res2.dtype == F32 else 0
    if master is not None:
        _req(master, F32, "master")
        if master.shape != (m_out, n_out) or geglu:
            raise ValueError("gemm: master must be f32 [M, N] (not available with GEGLU)")
        d.out_master, d.ldm = _p(master), _ld(master)
    d.alpha = alpha
    d.mode = mode
    if rowstats is not None:
        _req(rowstats, F32, "rowstats")
        if not rowstats.is_contiguous() or rowstats.numel() != M * (N // 32) * 2:
            raise ValueError("gemm: rowstats must be contiguous f32 [M, N/32, 2]")
        d.rowstats = _p(rowstats)
        d.flags |= ROWSTATS
    # A-resident N-streaming tile (csrc/nstream.hip): decided HERE, once — the caller passes the fragment-ordered copy and the raw K / 32
    # statistics; when the tile does not apply (planes / split mode, M too small, a non-contiguous copy) the product runs on the table's
    # tiles, and the GEGLU projection's statistics are pre-folded (avsd_ln_fold) so that they are not re-folded in every column tile
    x2_now = P.SPLIT or planes
    use_nstream = False
    if tile == NSTREAM_TILE or (tile == 0 and _NSTREAM and w_frag is not None):
        use_nstream = (w_frag is not None and not x2_now and mode == PLAIN and a2 is None and split_k == 1 and K in (320, 640) and N % 32 == 0
                       and (tile == NSTREAM_TILE or nstream_supported(M, N, K))
                       and stats_pos is None and ln_pos is None and w_frag.dtype == P.ACT and w_frag.is_contiguous() and w_frag.numel() == N * K)
        if tile == NSTREAM_TILE and not use_nstream:
            raise ValueError("gemm: tile 70 needs w_frag (weights.pack_frag) and a PLAIN single-source product with K = 320 / 640, N % 32 == 0")
    if w_frag is not None and not use_nstream and ln is not None and geglu and ln[0].shape[-2] != 1 and ln_pos is None:
        ln = (ln_fold(ln[0]), ln[1], ln[2])
    if ln is not None:
        st, colsum, eps = ln
        _req(st, F32, "ln stats")
        _req(colsum, F32, "ln colsum")
        if not st.is_contiguous() or st.shape[-2:] not in ((K // 32, 2), (1, 2)) or colsum.numel() != N:
            raise ValueError("gemm: ln = (stats [rows, K/32, 2], colsum [N], eps)")
        d.ln_stats, d.ln_colsum, d.ln_nblk, d.ln_eps = _p(st), _p(colsum), st.shape[-2], float(eps)
        d.flags |= LNFUSE
    for name, arg in (("stats_pos", stats_pos), ("ln_pos", ln_pos)):
        if arg is None:
            continue
        tbl, hw_, fr_ = arg
        _req(tbl, F32, name)
        if P.SPLIT or not tbl.is_contiguous() or tbl.shape != (fr_, N) or hw_ <= 0 or (rowstats is None if name == "stats_pos" else ln is None):
            raise ValueError(f"gemm: {name} = (f32 [frames, N], hw, frames) goes with " + ("rowstats" if name == "stats_pos" else "ln") +
                             "; not in split precision")
        if name == "stats_pos":
            d.stats_pos = _p(tbl)
        else:
            d.ln_rowvec = _p(tbl)
        d.pos_hw, d.pos_frames = int(hw_), int(fr_)
    # XCD banding: the 8 L2s are not shared, so whichever operand is NOT banded is fetched by all 8 of them
    a_bytes = M * (K // (4 if d.ups == 2 else 9) if mode == CONV3 else K // 3 if mode == TMIX else K)
    if _XCD_MODE == "n" or (_XCD_MODE == "auto" and N * K > a_bytes):
        d.flags |= XCD_N
    d.batch = 1
    d.raster_g = _RASTER_G
    ws = None
    key_flags, key_master = None, int(master is not None)
    if planes:
        d.flags |= X2
        d.a_lo, d.a2_lo, d.w_lo = _rest_off(a, a_rest), (_rest_off(a2, a2_rest) if a2 is not None else 0), _rest_off(w, w_rest)
        if out_rest is not None:
            # (main, rest) planes (+ f32 master) instead of f32: the same main loop — the tile table keeps ONE entry per three-pass shape
            d.out_lo = _rest_off(out, out_rest)
            key_flags, key_master = d.flags | OUT_F32, 0
    elif out_rest is not None:
        key_flags = d.flags                 # (the rest-plane store does not change which tile is fastest: not part of the table key)
        d.flags |= OUT_REST
        d.out_lo = _rest_off(out, out_rest)
    elif P.SPLIT:
        if master is not None:
            raise ValueError("gemm: split precision has no f32 master (the planes carry 16 bits)")
        d.flags |= X2
        d.a_lo, d.a2_lo, d.w_lo = _lo(a), _lo(a2), _lo(w)
        d.out_lo = 0 if out_f32 else _lo(out)
        d.res1_lo = _lo(res1) if (res1 is not None and res1.dtype != F32) else 0
        d.res2_lo = _lo(res2) if (res2 is not None and res2.dtype != F32) else 0

    if use_nstream:
        tile = NSTREAM_TILE
        d.W = _p(w_frag)
        d.flags |= W_FRAG

    def _set(t, sk):
        nonlocal ws
        d.tile, d.split_k = t, sk
        krot = _KROT and (t in ASM_TILES or not _KROT_ASM_ONLY) and 2 * N * K <= _KROT_MAX_W
        d.flags = (d.flags | KROT) if krot else (d.flags & ~KROT)          # (set after the table key was formed: not part of it)
        if sk > 1:
            if ws is None or ws.numel() < sk * M * N:
                ws = torch.empty((sk * M * N,), dtype=F32, device=a.device)
            d.splitk_ws = _p(ws)

    if tile == 0:
        def _launch(t, sk):
            _set(t, sk)
            check(_lib.lib().avsd_gemm_bf16(C.byref(d), _stream()), "avsd_gemm_bf16")

        cands = X2_TILE_CANDIDATES if x2 else TILE_CANDIDATES
        nk = (K + 63) // 64
        two_src_unaligned = a2 is not None and (a.shape[1] % 64 != 0)     # C falls back to register-staged tiles
        if not geglu and not two_src_unaligned and ((M + 127) // 128) * ((N + 127) // 128) < 256 and nk >= 16:
            cands = cands + tuple(c for c in (X2_SPLITK_CANDIDATES if x2 else SPLITK_CANDIDATES) if nk // c[1] >= 4)
        splitk_ok = not geglu and not two_src_unaligned
        if mode == CONV3 and d.ups == 2:       # the tiles built for this loader whose column tiles do not straddle two output-pixel parities
            ok_tiles = SUBPIX_X2_TILES if x2 else SUBPIX_TILES
            cands = tuple(c for c in cands if c[0] in ok_tiles and (N // 4) % TILE_BN[c[0]] == 0)
        two_src_conv = mode == CONV3 and a2 is not None           # only the LDS-resident tiles read a second source
        if two_src_conv:
            cands = conv3r_candidates(d.hs, d.ws, d.cin, M, N)
            if not cands:
                raise ValueError("gemm: no LDS-resident convolution tile takes this two-source geometry")
        elif (_CONV3R and mode == CONV3 and not x2 and d.stride == 1 and d.ups == 0 and d.pad == 1 and ln is None and out_rest is None):
            cands = cands + conv3r_candidates(d.hs, d.ws, d.cin, M, N)
        # 16-bit convolutions are keyed by the image geometry too: which LDS-resident tiles apply depends on (hs, ws)
        key = (mode, M, N, K, d.flags if key_flags is None else key_flags, d.stride, d.ups, d.pad, key_master)
        if mode == CONV3 and not x2:
            key = key + (d.hs, d.ws)
        if two_src_conv:
            key = key + ("a2", d.k_split)                         # a table entry of the one-source shape may name a tile that never reads A2
        asm = ()
        if (_ASM_TILES and a2 is None and K % 64 == 0 and M * lda < (1 << 29) and N * _ld(w) < (1 << 29) and
                (mode == PLAIN or (mode == TMIX and d.cseg % 64 == 0 and ln is None))):
            asm = ASM_X2_CANDIDATES if x2 else tuple(c for c in ASM_CANDIDATES if mode == PLAIN or c[0] != 60)
            if splitk_ok and ((M + 127) // 128) * ((N + 127) // 128) < 256 and nk >= 8:
                asm = asm + tuple(c for c in (ASM_X2_SPLITK_CANDIDATES if x2 else ASM_SPLITK_CANDIDATES)
                                  if nk // c[1] >= 4 and (c[1] - 1) * -(-nk // c[1]) < nk)      # (no empty K slice: the asm tiles refuse it)
        if RECORD_KEYS is not None:          # tools/tune_in_step.py: which table keys a forward uses, how often, and what could run them
            rec = RECORD_KEYS.setdefault(key, {"n": 0, "cands": tuple(dict.fromkeys(tuple(cands) + tuple(asm))), "flops": 2.0 * M * N * K})
            rec["n"] += 1
        picked = _pick_tile(key, _launch, cands, warm=(a, a2, res1, res2), challengers=asm)
        if picked is not None and picked[0] in ASM_TILES and not asm:        # (a two-source call shares the key of the one-source shape)
            picked = None
        if picked is not None and picked[0] in CONV3R_TILES and not ((_CONV3R or two_src_conv) and _lib.lib().avsd_gemm_conv3r_supported(picked[0], d.hs, d.ws, d.cin)):
            picked = None
        if picked is not None and picked[0] in CONV3R2D_TILES and not ((_CONV3R or two_src_conv) and _lib.lib().avsd_gemm_conv3r2d_supported(picked[0], d.hs, d.ws, d.cin)):
            picked = None
        if picked is not None and two_src_conv and picked not in cands:
            picked = None
        if picked is not None and out_rest is not None and not planes and (picked[0] in CONV3R_TILES or picked[0] in CONV3R2D_TILES):
            picked = None            # (the LDS-resident convolution tiles have no rest-plane store)
        heur = _heuristic_tile_x2 if x2 else _heuristic_tile
        if picked is None and two_src_conv:
            picked = _heuristic_conv3r(cands, M, N)
        tile, split_k = picked if picked is not None else heur(M, N, K, geglu, splitk_ok)
        if mode == CONV3 and d.ups == 2:
            tile = _subpix_tile(tile, N // 4, x2)      # (the rule may name a tile this loader is not built for, or one wider than a divisor of cout)
    _set(tile, split_k)
    ev = _TIMER.start() if _TIMER is not None else None
    check(_lib.lib().avsd_gemm_bf16(C.byref(d), _stream()), "avsd_gemm_bf16")
    if ev is not None:
        fam = ("gemm_plain", "gemm_tmix", "gemm_conv3")[mode]
        dc = GemmDesc.from_buffer_copy(d)
        _TIMER.add_replay(fam, lambda dc=dc: check(_lib.lib().avsd_gemm_bf16(C.byref(dc), _stream()), "avsd_gemm_bf16"),
                          (a, a2, w, out, bias, rowvec, res1, res2, ws, rowstats, ln, master, stats_pos, ln_pos, a_rest, a2_rest, w_rest, w_frag, out_rest))
        subpix = mode == CONV3 and d.ups == 2
        _TIMER.stop(ev, fam, 2.0 * M * N * K * (3 if x2 else 1), 2.0 * M * K * (1.0 / (4 if subpix else 9) if mode == CONV3 else 1.0 / 3 if mode == TMIX else 1.0)
                    + 2.0 * N * K + _nbytes(out, res1, res2), flops_once=2.0 * M * N * K, flops_ref=2.0 * M * N * K * (2.25 if subpix else 1.0))
    return out


def gemm_f32(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """exact-f32 yardstick: out = a . w^T + bias on v_mfma_f32_32x32x2_f32 (avsd_gemm_f32); a [M, K], w [N, K] f32"""
    _req(a, F32, "a")
    _req(w, F32, "w")
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=F32, device=a.device)
    check(_lib.lib().avsd_gemm_f32(_p(a), _ld(a), _p(w), _ld(w), _p(bias), _p(out), _ld(out), M, N, K, _stream()), "avsd_gemm_f32")
    return out


def gemm_batched(a: torch.Tensor, w: torch.Tensor, *, alpha: float = 1.0, out_f32: bool = False,
                 bias: Optional[torch.Tensor] = None, tile: int = 0, ln: Optional[tuple] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b] = alpha * a[b] . w[b]^T for 3-D a [B, M, K], w [B, N, K] (VAE mid-block attention).  `out`: [B, M, N] of the output type, rows
    contiguous (any row and batch stride the descriptor's alignment rules admit)."""
    _req(a, P.ACT, "a")
    _req(w, P.ACT, "w")
    B, M, K = a.shape
    N = w.shape[1]
    if out is None:
        out = torch.empty((B, M, N), dtype=F32, device=a.device) if out_f32 else alloc16((B, M, N), a.device)
    else:
        _req(out, F32 if out_f32 else P.ACT, "out")
        if tuple(out.shape) != (B, M, N):
            raise ValueError(f"gemm_batched: out must be [{B}, {M}, {N}], got {tuple(out.shape)}")
    d = GemmDesc()
    d.A, d.W, d.out = _p(a), _p(w), _p(out)
    d.M, d.N, d.K, d.k_split = M, N, K, K
    d.lda, d.ldw, d.ldc = a.stride(1), w.stride(1), out.stride(1)
    d.alpha, d.mode, d.flags, d.batch, d.tile = alpha, PLAIN, (OUT_F32 if out_f32 else 0), B, tile
    d.batch_stride_a, d.batch_stride_w, d.batch_stride_out = a.stride(0), w.stride(0), out.stride(0)
    if bias is not None:
        _req(bias, F32, "bias")
        d.bias = _p(bias)
    if ln is not None:          # statistics are indexed by the row of the full tensor the batches are views of
        st, colsum, eps = ln
        _req(st, F32, "ln stats")
        _req(colsum, F32, "ln colsum")
        d.ln_stats, d.ln_colsum, d.ln_nblk, d.ln_eps = _p(st), _p(colsum), K // 32, float(eps)
        d.flags |= LNFUSE
    if P.SPLIT:
        d.flags |= X2
        d.a_lo, d.w_lo, d.out_lo = _lo(a), _lo(w), (0 if out_f32 else _lo(out))
    if tile == 0:
        def _launch(t):
            d.tile = t
            check(_lib.lib().avsd_gemm_bf16(C.byref(d), _stream()), "avsd_gemm_bf16(batched)")

        picked = _pick_tile(("batched", B, M, N, K, d.flags), lambda t, sk: _launch(t), X2_TILE_CANDIDATES if P.SPLIT else TILE_CANDIDATES)
        d.tile = picked[0] if picked is not None else (_heuristic_tile_x2 if P.SPLIT else _heuristic_tile)(B * M, N, K, False, False)[0]
    dc = GemmDesc.from_buffer_copy(d) if _TIMER is not None else d
    _timed("gemm_plain", 2.0 * B * M * N * K * (3 if P.SPLIT else 1), 2.0 * B * (M * K + N * K) + _nbytes(out), (a, w, out, bias, ln),
           lambda: check(_lib.lib().avsd_gemm_bf16(C.byref(dc), _stream()), "avsd_gemm_bf16(batched)"))
    return out


def linear_small_m(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], *, act_in: bool = False,
                   act_out: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req(x, F32, "x")
    _req(w, P.ACT, "w")
    M, K = x.shape
    N = w.shape[0]
    if not x.is_contiguous():
        raise ValueError("linear_small_m: x must be contiguous")
    if out is None:
        out = torch.empty((M, N), dtype=F32, device=x.device)
    if P.SPLIT:
        check(_lib.lib().avsd_linear_small_m_x2(_p(x), _p(w), _lo(w), _p(bias), _p(out), M, N, K, _ld(w), int(act_in), int(act_out),
                                                _stream()), "avsd_linear_small_m_x2")
        return out
    check(_lib.lib().avsd_linear_small_m(_p(x), _p(w), _p(bias), _p(out), M, N, K, _ld(w), int(act_in), int(act_out),
                                         _stream()), "avsd_linear_small_m")
    return out


# one-launch GroupNorm for small batches (csrc/groupnorm_fused.hip); AVSD_GN_FUSED=0: always the pair
_GN_FUSED = True

def groupnorm(x1: torch.Tensor, x2: Optional[torch.Tensor], nb: int, rows_per_batch: int, groups: int,
              gamma: torch.Tensor, beta: torch.Tensor, eps: float, act: bool,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GroupNorm(+SiLU) of the channel concat [x1 | x2]; statistics pooled over each run of
    `rows_per_batch` rows.  One launch for small batches (avsd_groupnorm_fused: the ResBlock norms at 4 x 4, the per-frame
    norms up to 16 x 16), else two: partial sums, then reduce + apply."""
    _req(x1, P.ACT, "x1")
    c1 = x1.shape[1]
    c2 = 0
    if x2 is not None:
        _req(x2, P.ACT, "x2")
        c2 = x2.shape[1]
    _req(gamma, F32, "gamma")
    _req(beta, F32, "beta")
    L = _lib.lib()
    rows = nb * rows_per_batch
    if out is None:
        out = alloc16((rows, c1 + c2), x1.device)
    ld2 = _ld(x2) if x2 is not None else 0
    keep = (x1, x2, gamma, beta, out)
    if _GN_FUSED and L.avsd_groupnorm_fused_supported(nb, rows_per_batch, groups, c1, c2, int(P.SPLIT)):
        if P.SPLIT:
            a_ = (_p(x1), _ld(x1), c1, _lo(x1), _p(x2), ld2, c2, _lo(x2), nb, rows_per_batch, groups, _p(gamma), _p(beta), float(eps), int(act),
                  _p(out), _ld(out), _lo(out))
            _timed("groupnorm", 0.0, _nbytes(x1, x2) + _nbytes(out), keep, lambda: check(L.avsd_groupnorm_fused_x2(*a_, _stream()), "avsd_groupnorm_fused_x2"))
        else:
            a_ = (_p(x1), _ld(x1), c1, _p(x2), ld2, c2, nb, rows_per_batch, groups, _p(gamma), _p(beta), float(eps), int(act), _p(out), _ld(out))
            _timed("groupnorm", 0.0, _nbytes(x1, x2) + _nbytes(out), keep, lambda: check(L.avsd_groupnorm_fused(*a_, _stream()), "avsd_groupnorm_fused"))
        return out
    nchunks = L.avsd_groupnorm_nchunks(nb, rows_per_batch, c1 + c2)
    partial = torch.empty((L.avsd_groupnorm_scratch_floats(nb, nchunks, groups, c1 + c2),), dtype=F32, device=x1.device)
    keep = keep + (partial,)
    if P.SPLIT:
        s_ = (_p(x1), _ld(x1), c1, _lo(x1), _p(x2), ld2, c2, _lo(x2), nb, rows_per_batch, groups, _p(partial), nchunks)
        a_ = (_p(x1), _ld(x1), c1, _lo(x1), _p(x2), ld2, c2, _lo(x2), nb, rows_per_batch, groups, _p(gamma), _p(beta), float(eps), _p(partial),
              nchunks, int(act), _p(out), _ld(out), _lo(out))
        _timed("groupnorm", 0.0, 2.0 * _nbytes(x1, x2) + _nbytes(out), keep,
               lambda: check(L.avsd_groupnorm_stats_x2(*s_, _stream()), "avsd_groupnorm_stats_x2"),
               lambda: check(L.avsd_groupnorm_apply_x2(*a_, _stream()), "avsd_groupnorm_apply_x2"))
    else:
        s_ = (_p(x1), _ld(x1), c1, _p(x2), ld2, c2, nb, rows_per_batch, groups, _p(partial), nchunks)
        a_ = (_p(x1), _ld(x1), c1, _p(x2), ld2, c2, nb, rows_per_batch, groups, _p(gamma), _p(beta), float(eps), _p(partial), nchunks, int(act),
              _p(out), _ld(out))
        _timed("groupnorm", 0.0, 2.0 * _nbytes(x1, x2) + _nbytes(out), keep,
               lambda: check(L.avsd_groupnorm_stats(*s_, _stream()), "avsd_groupnorm_stats"),
               lambda: check(L.avsd_groupnorm_apply(*a_, _stream()), "avsd_groupnorm_apply"))
    return out


def groupnorm_planes(x1: torch.Tensor, x1_rest: torch.Tensor, nb: int, rows_per_batch: int, groups: int, gamma: torch.Tensor,
                     beta: torch.Tensor, eps: float, act: bool):
    """GroupNorm(+SiLU) of a two-plane tensor into two planes, whatever the process-wide mode: the input of a three-pass product under
    the per-layer precision plan (conv_out reads conv_norm_out's result).  -> (main, rest)"""
    _req(x1, P.ACT, "x1")
    L = _lib.lib()
    c1 = x1.shape[1]
    out, out_rest = alloc_planes((nb * rows_per_batch, c1), x1.device)
    lo_in, lo_out = _rest_off(x1, x1_rest), _rest_off(out, out_rest)
    nchunks = L.avsd_groupnorm_nchunks(nb, rows_per_batch, c1)
    partial = torch.empty((L.avsd_groupnorm_scratch_floats(nb, nchunks, groups, c1),), dtype=F32, device=x1.device)
    s_ = (_p(x1), _ld(x1), c1, lo_in, None, 0, 0, 0, nb, rows_per_batch, groups, _p(partial), nchunks)
    a_ = (_p(x1), _ld(x1), c1, lo_in, None, 0, 0, 0, nb, rows_per_batch, groups, _p(gamma), _p(beta), float(eps), _p(partial), nchunks, int(act),
          _p(out), _ld(out), lo_out)
    _timed("groupnorm", 0.0, 4.0 * _nbytes(x1) + 2.0 * _nbytes(out), (x1, x1_rest, gamma, beta, out, out_rest, partial),
           lambda: check(L.avsd_groupnorm_stats_x2(*s_, _stream()), "avsd_groupnorm_stats_x2"),
           lambda: check(L.avsd_groupnorm_apply_x2(*a_, _stream()), "avsd_groupnorm_apply_x2"))
    return out, out_rest


def ncfhw_to_rows_planes(x: torch.Tensor, cpad: int, rep: int = 1, scale: float = 1.0):
    """ncfhw_to_rows into (main, rest) planes, whatever the process-wide mode (conv_in as a three-pass product)"""
    _req(x, F32, "x")
    if not x.is_contiguous():
        raise ValueError("ncfhw_to_rows: x must be contiguous")
    B, Cc, Fr, H, W = x.shape
    out, rest = alloc_planes((rep * B * Fr * H * W, cpad), x.device)
    check(_lib.lib().avsd_ncfhw_to_rows_x2(_p(x), _p(out), _rest_off(out, rest), B, Cc, Fr, H * W, cpad, rep, float(scale), _stream()),
          "avsd_ncfhw_to_rows_x2")
    return out, rest


def ln_fold(stats: torch.Tensor) -> torch.Tensor:
    """row statistics [M, K/32, 2] of a ROWSTATS producer -> [M, 1, 2]: the pair a LayerNorm-folding consumer (gemm(ln=...)) would fold
    itself in every column tile, folded once (same order, same bits)"""
    _req(stats, F32, "stats")
    M, nblk = stats.shape[0], stats.shape[1]
    out = torch.empty((M, 1, 2), dtype=F32, device=stats.device)
    _timed("ln_fold", 0.0, _nbytes(stats, out), (stats, out), lambda: check(_lib.lib().avsd_ln_fold(_p(stats), M, nblk, _p(out), _stream()), "avsd_ln_fold"))
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
              pos: Optional[torch.Tensor] = None, hw: int = 1, frames: int = 1,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req(x, P.ACT, "x")
    _req(gamma, F32, "gamma")
    _req(beta, F32, "beta")
    M, Cc = x.shape
    if pos is not None:
        _req(pos, F32, "pos")
        if not pos.is_contiguous() or pos.shape != (frames, Cc):
            raise ValueError("layernorm: pos must be contiguous [frames, C]")
    if out is None:
        out = alloc16((M, Cc), x.device)
    if P.SPLIT:
        a_ = (_p(x), _ld(x), _lo(x), _p(out), _ld(out), _lo(out), M, Cc, _p(gamma), _p(beta), float(eps), _p(pos), hw, frames)
        call = lambda: check(_lib.lib().avsd_layernorm_x2(*a_, _stream()), "avsd_layernorm_x2")   # noqa: E731
    else:
        a_ = (_p(x), _ld(x), _p(out), _ld(out), M, Cc, _p(gamma), _p(beta), float(eps), _p(pos), hw, frames)
        call = lambda: check(_lib.lib().avsd_layernorm(*a_, _stream()), "avsd_layernorm")   # noqa: E731
    _timed("layernorm", 0.0, _nbytes(x, out), (x, out, gamma, beta, pos), call)
    return out


def softmax_rows(s: torch.Tensor) -> torch.Tensor:
    _req(s, F32, "s")
    rows, L = s.shape
    out = alloc16((rows, L), s.device)
    check(_lib.lib().avsd_softmax_rows_x2(_p(s), _ld(s), _p(out), _ld(out), _lo(out), rows, L, _stream()), "avsd_softmax_rows_x2")
    return out


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, bq: int, lq: int, lk: int, kv_rows: int,
              heads: int, q_per_kv: int, frames: int, key_index: Optional[torch.Tensor] = None,
              scale: Optional[float] = None, out: Optional[torch.Tensor] = None, fp8: Optional[tuple] = None) -> torch.Tensor:
    """q [bq*lq, heads*d]; k, v [(bq/q_per_kv)*kv_rows, >= heads*d] (views into a fused k|v buffer are fine).
    fp8 = (q_scale, k_scale, v_scale): the e4m3 Q/K/V kernel (avsd_attention_fp8, BASELINE cfg 5) instead of the 16-bit one."""
    _req(q, P.ACT, "q")
    _req(k, P.ACT, "k")
    _req(v, P.ACT, "v")
    Cc = q.shape[1]
    d = Cc // heads
    if key_index is not None:
        if key_index.dtype != torch.int32 or not key_index.is_contiguous() or key_index.shape != (frames, lk):
            raise ValueError("attention: key_index must be contiguous int32 [frames, lk]")
    if out is None:
        out = alloc16((bq * lq, Cc), q.device)
    if scale is None:
        scale = float(d) ** -0.5
    if P.SPLIT:
        if fp8 is not None:
            raise ValueError("attention: fp8 Q/K/V and split precision are exclusive")
        a_ = (_p(q), _ld(q), _lo(q), _p(k), _ld(k), _lo(k), _p(v), _ld(v), _lo(v), _p(out), _ld(out), _lo(out), bq, lq, lk, kv_rows, heads, d,
              q_per_kv, _p(key_index), frames, float(scale))
        call = lambda: check(_lib.lib().avsd_attention_x2(*a_, _stream()), "avsd_attention_x2")   # noqa: E731
    elif fp8 is not None:
        qs, ks, vs = (float(x) for x in fp8)
        a_ = (_p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(out), _ld(out), bq, lq, lk, kv_rows, heads, d, q_per_kv, _p(key_index), frames,
              float(scale), qs, ks, vs)
        call = lambda: check(_lib.lib().avsd_attention_fp8(*a_, _stream()), "avsd_attention_fp8")   # noqa: E731
    else:
        a_ = (_p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(out), _ld(out), bq, lq, lk, kv_rows, heads, d, q_per_kv, _p(key_index), frames,
              float(scale))
        call = lambda: check(_lib.lib().avsd_attention(*a_, _stream()), "avsd_attention")   # noqa: E731
    _timed("attention", 4.0 * bq * heads * lq * lk * d * (3 if P.SPLIT else 1), _nbytes(q, out) + 4.0 * (bq // q_per_kv) * lk * Cc,
           (q, k, v, out, key_index), call)
    return out


def cross_attention_block_supported(C: int, heads: int, lk_pad: int, M: int, L: int) -> bool:
    return not P.SPLIT and bool(_lib.lib().avsd_cross_attention_block_supported(C, heads, lk_pad)) and M % 128 == 0 and L % 128 == 0


def cross_attention_block(h: torch.Tensor, stats: torch.Tensor, wq: torch.Tensor, q_colsum: torch.Tensor, q_bias: torch.Tensor,
                          k: torch.Tensor, vt: torch.Tensor, lk: int, wo: torch.Tensor, o_bias: torch.Tensor, *, res: torch.Tensor,
                          heads: int, L: int, q_per_kv: int, eps: float = 1e-5, scale: Optional[float] = None,
                          rowstats: Optional[torch.Tensor] = None, master: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None, stats_pos: Optional[tuple] = None) -> torch.Tensor:
    """out = res + to_out(softmax((LN(h) Wq^T) K^T scale) V) in one launch; see avsd_cross_attention_block (include/avsd.h).
    k [nkv, lk_pad, C], vt [nkv, C, lk_pad] are the cached, padded (and for audio mask-gathered) K / V^T."""
    if P.SPLIT:
        raise ValueError("cross_attention_block: not built for split precision (use the separate kernels)")
    _req(h, P.ACT, "h")
    _req(wq, P.ACT, "wq")
    _req(wo, P.ACT, "wo")
    _req(k, P.ACT, "k")
    _req(vt, P.ACT, "vt")
    _req(stats, F32, "stats")
    M, Cc = h.shape
    lk_pad = k.shape[1]
    if not k.is_contiguous() or not vt.is_contiguous() or vt.shape != (k.shape[0], Cc, lk_pad) or k.shape[2] != Cc:
        raise ValueError("cross_attention_block: k must be contiguous [nkv, lk_pad, C] and vt [nkv, C, lk_pad]")
    if not stats.is_contiguous() or stats.shape != (M, Cc // 32, 2):
        raise ValueError("cross_attention_block: stats must be contiguous f32 [M, C/32, 2]")
    if (M // L) // q_per_kv > k.shape[0] or (M // L) % q_per_kv:
        raise ValueError("cross_attention_block: K/V blocks do not cover the query batches")
    if out is None:
        out = torch.empty((M, Cc), dtype=P.ACT, device=h.device)
    d = XAttnDesc()
    d.h, d.ldh = _p(h), _ld(h)
    _req(res, F32 if res.dtype == F32 else P.ACT, "res")
    d.res, d.ldres, d.res_f32 = _p(res), _ld(res), int(res.dtype == F32)
    d.M, d.C, d.heads, d.L = M, Cc, heads, L
    d.ln_stats, d.ln_eps = _p(stats), float(eps)
    d.scale = float(scale) if scale is not None else float(Cc // heads) ** -0.5
    d.wq, d.ldwq, d.q_colsum, d.q_bias = _p(wq), _ld(wq), _p(q_colsum), _p(q_bias)
    d.k, d.vt, d.lk, d.lk_pad, d.q_per_kv = _p(k), _p(vt), lk, lk_pad, q_per_kv
    d.wo, d.ldwo, d.o_bias = _p(wo), _ld(wo), _p(o_bias)
    d.out, d.ldo = _p(out), _ld(out)
    if master is not None:
        _req(master, F32, "master")
        d.out_master, d.ldm = _p(master), _ld(master)
    if rowstats is not None:
        _req(rowstats, F32, "rowstats")
        d.rowstats = _p(rowstats)
    if stats_pos is not None:
        tbl, hw_, fr_ = stats_pos
        _req(tbl, F32, "stats_pos")
        if rowstats is None or not tbl.is_contiguous() or tbl.shape != (fr_, Cc) or hw_ <= 0:
            raise ValueError("cross_attention_block: stats_pos = (f32 [frames, C], hw, frames) goes with rowstats")
        d.stats_pos, d.pos_hw, d.pos_frames = _p(tbl), int(hw_), int(fr_)
    ev = _TIMER.start() if _TIMER is not None else None
    check(_lib.lib().avsd_cross_attention_block(C.byref(d), _stream()), "avsd_cross_attention_block")
    if ev is not None:
        dc = XAttnDesc.from_buffer_copy(d)
        _TIMER.add_replay("cross_attention_block", lambda dc=dc: check(_lib.lib().avsd_cross_attention_block(C.byref(dc), _stream()),
                                                                         "avsd_cross_attention_block"),
                          (h, stats, wq, q_colsum, q_bias, k, vt, wo, o_bias, res, out, master, rowstats, stats_pos))
        _TIMER.stop(ev, "cross_attention_block", 4.0 * M * Cc * Cc + 4.0 * M * lk * Cc, _nbytes(h, out, res, master) + 4.0 * Cc * Cc)
    return out


def qproj_attention_supported(C: int, heads: int, lk_pad: int, M: int, L: int, q_per_kv: int) -> bool:
    """LayerNorm-folded Q projection + cross-attention as one launch (avsd_qproj_attention): the wider levels the fused block is not built for"""
    return (not P.SPLIT and L > 0 and q_per_kv > 0 and M % (L * q_per_kv) == 0
            and bool(_lib.lib().avsd_qproj_attention_supported(C, heads, lk_pad, L * q_per_kv)))


def qproj_attention(h: torch.Tensor, stats: torch.Tensor, wq: torch.Tensor, q_colsum: torch.Tensor, q_bias: torch.Tensor,
                    k: torch.Tensor, vt: torch.Tensor, lk: int, *, heads: int, L: int, q_per_kv: int, eps: float = 1e-5,
                    scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = softmax((LN(h) Wq^T) K^T scale) V in one launch; see avsd_qproj_attention (include/avsd.h).  Operands as
    cross_attention_block: k [nkv, lk_pad, C], vt [nkv, C, lk_pad] are the cached, padded K / V^T."""
    if P.SPLIT:
        raise ValueError("qproj_attention: not built for split precision (use the separate kernels)")
    _req(h, P.ACT, "h")
    _req(wq, P.ACT, "wq")
    _req(k, P.ACT, "k")
    _req(vt, P.ACT, "vt")
    _req(stats, F32, "stats")
    _req(q_colsum, F32, "q_colsum")
    _req(q_bias, F32, "q_bias")
    M, Cc = h.shape
    if k.dim() != 3 or not k.is_contiguous() or not vt.is_contiguous() or vt.shape != (k.shape[0], Cc, k.shape[1]) or k.shape[2] != Cc:
        raise ValueError("qproj_attention: k must be contiguous [nkv, lk_pad, C] and vt [nkv, C, lk_pad]")
    lk_pad = k.shape[1]
    if not stats.is_contiguous() or stats.shape != (M, Cc // 32, 2):
        raise ValueError("qproj_attention: stats must be contiguous f32 [M, C/32, 2]")
    if wq.shape != (Cc, Cc) or q_colsum.numel() != Cc or q_bias.numel() != Cc or not q_colsum.is_contiguous() or not q_bias.is_contiguous():
        raise ValueError("qproj_attention: wq [C, C] with q_colsum [C] and q_bias [C] expected")
    if L <= 0 or q_per_kv <= 0 or M % L or (M // L) % q_per_kv or (M // L) // q_per_kv > k.shape[0]:
        raise ValueError("qproj_attention: K/V blocks do not cover the query batches")
    if out is None:
        out = torch.empty((M, Cc), dtype=P.ACT, device=h.device)
    _req(out, P.ACT, "out")
    if out.shape != (M, Cc):
        raise ValueError("qproj_attention: out must be [M, C]")
    d = XAttnDesc()
    d.h, d.ldh = _p(h), _ld(h)
    d.M, d.C, d.heads, d.L = M, Cc, heads, L
    d.ln_stats, d.ln_eps = _p(stats), float(eps)
    d.scale = float(scale) if scale is not None else float(Cc // heads) ** -0.5
    d.wq, d.ldwq, d.q_colsum, d.q_bias = _p(wq), _ld(wq), _p(q_colsum), _p(q_bias)
    d.k, d.vt, d.lk, d.lk_pad, d.q_per_kv = _p(k), _p(vt), lk, lk_pad, q_per_kv
    d.out, d.ldo = _p(out), _ld(out)
    ev = _TIMER.start() if _TIMER is not None else None
    check(_lib.lib().avsd_qproj_attention(C.byref(d), _stream()), "avsd_qproj_attention")
    if ev is not None:
        dc = XAttnDesc.from_buffer_copy(d)
        _TIMER.add_replay("qproj_attention", lambda dc=dc: check(_lib.lib().avsd_qproj_attention(C.byref(dc), _stream()), "avsd_qproj_attention"),
                          (h, stats, wq, q_colsum, q_bias, k, vt, out))
        _TIMER.stop(ev, "qproj_attention", 2.0 * M * Cc * Cc + 4.0 * M * lk * Cc, _nbytes(h, out) + 2.0 * Cc * Cc)
    return out


def ff_block_supported(M: int, C: int, with_proj_out: bool = True) -> bool:
    """GEGLU projection + FF-out (+ proj_out) of a transformer block as one launch (avsd_ff_block): where it is built and measured
    faster than the launches it replaces"""
    return not P.SPLIT and bool(_lib.lib().avsd_ff_block_supported(M, C, int(with_proj_out)))


def ff_block(h: torch.Tensor, stats: torch.Tensor, w1_frag: torch.Tensor, w1_colsum: torch.Tensor, b1: torch.Tensor,
             w2_frag: torch.Tensor, b2: torch.Tensor, wp_frag: Optional[torch.Tensor] = None, bp: Optional[torch.Tensor] = None,
             x: Optional[torch.Tensor] = None, *, eps: float = 1e-5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = (GEGLU(LN(h) W1'^T + b1) W2^T + b2 + h) Wp^T + bp + x in one launch, or without wp_frag the inner h' alone; see
    avsd_ff_block (include/avsd.h).  The three weights come in MFMA-fragment order (weights.pack_frag), W1' packed for GEGLU with the
    LayerNorm gain folded in, w1_colsum / b1 as the LayerNorm-folded GEMM takes them; stats [M, C / 32, 2] or pre-folded [M, 1, 2]."""
    if P.SPLIT:
        raise ValueError("ff_block: not built for split precision (use the separate kernels)")
    _req(h, P.ACT, "h")
    _req(stats, F32, "stats")
    for t, nm in ((w1_frag, "w1_frag"), (w2_frag, "w2_frag")) + (((wp_frag, "wp_frag"),) if wp_frag is not None else ()):
        _req(t, P.ACT, nm)
    for t, nm in ((w1_colsum, "w1_colsum"), (b1, "b1"), (b2, "b2")) + (((bp, "bp"),) if bp is not None else ()):
        _req(t, F32, nm)
    if h.dim() != 2:
        raise ValueError("ff_block: h must be [M, C]")
    M, Cc = h.shape
    if (not w1_frag.is_contiguous() or not w2_frag.is_contiguous() or w1_frag.numel() != 8 * Cc * Cc or w2_frag.numel() != 4 * Cc * Cc
            or w1_colsum.numel() != 8 * Cc or b1.numel() != 8 * Cc or b2.numel() != Cc
            or not (w1_colsum.is_contiguous() and b1.is_contiguous() and b2.is_contiguous())):
        raise ValueError("ff_block: w1_frag [8 C / 32, C / 16, 64, 8] with w1_colsum [8 C], b1 [8 C]; w2_frag [C / 32, 4 C / 16, 64, 8] with b2 [C]")
    if not stats.is_contiguous() or stats.dim() != 3 or stats.shape[0] != M or stats.shape[2] != 2:
        raise ValueError("ff_block: stats must be contiguous f32 [M, C / 32 or 1, 2]")
    if wp_frag is not None:
        if bp is None or x is None:
            raise ValueError("ff_block: wp_frag goes with bp and x")
        _req(x, P.ACT, "x")
        if not wp_frag.is_contiguous() or wp_frag.numel() != Cc * Cc or bp.numel() != Cc or not bp.is_contiguous() or x.shape != (M, Cc):
            raise ValueError("ff_block: wp_frag [C / 32, C / 16, 64, 8] with bp [C] and x [M, C]")
    if out is None:
        out = torch.empty((M, Cc), dtype=P.ACT, device=h.device)
    _req(out, P.ACT, "out")
    if out.shape != (M, Cc):
        raise ValueError("ff_block: out must be [M, C]")
    proj = wp_frag is not None
    a_ = (_p(h), _ld(h), _p(stats), int(stats.shape[1]), float(eps), _p(w1_frag), _p(w1_colsum), _p(b1), _p(w2_frag), _p(b2),
          _p(wp_frag), _p(bp) if proj else None, _p(x) if proj else None, _ld(x) if proj else 0, _p(out), _ld(out), M, Cc)
    _timed("ff_block", (24.0 + (2.0 if proj else 0.0)) * M * Cc * Cc, _nbytes(h, out, x if proj else None) + (24.0 + (2.0 if proj else 0.0)) * Cc * Cc,
           (h, stats, w1_frag, w1_colsum, b1, w2_frag, b2, wp_frag, bp, x, out),
           lambda: check(_lib.lib().avsd_ff_block(*a_, _stream()), "avsd_ff_block"))
    return out


def temporal_block_supported(M: int, C: int, heads: int, frames: int) -> bool:
    """q|k|v projection + temporal attention + output projection of a transformer block as one launch (avsd_temporal_block): where it
    is built and measured faster than the launches it replaces"""
    return not P.SPLIT and bool(_lib.lib().avsd_temporal_block_supported(M, C, heads, frames))


def temporal_block(h: torch.Tensor, stats: torch.Tensor, wqkv_frag: torch.Tensor, qkv_colsum: torch.Tensor, qkv_bias: torch.Tensor,
                   posw: torch.Tensor, wo_frag: torch.Tensor, bo: torch.Tensor, *, b: int, frames: int, hw: int, heads: int,
                   eps: float = 1e-5, scale: Optional[float] = None, rowstats: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = attention(LN(h + pos) Wqkv'^T + b) Wo^T + bo + h over the frames of each pixel, in one launch (+ the LayerNorm row
    statistics of out); see avsd_temporal_block (include/avsd.h).  wqkv_frag, qkv_colsum, qkv_bias and posw come in the regrouped
    q|k|v column order (weights.group_qkv), both weights in MFMA-fragment order (weights.pack_frag); stats [M, C / 32, 2] (of h + pos)
    or pre-folded [M, 1, 2]."""
    if P.SPLIT:
        raise ValueError("temporal_block: not built for split precision (use the separate kernels)")
    _req(h, P.ACT, "h")
    _req(stats, F32, "stats")
    _req(wqkv_frag, P.ACT, "wqkv_frag")
    _req(wo_frag, P.ACT, "wo_frag")
    for t, nm in ((qkv_colsum, "qkv_colsum"), (qkv_bias, "qkv_bias"), (posw, "posw"), (bo, "bo")):
        _req(t, F32, nm)
    if h.dim() != 2 or h.shape[0] != b * frames * hw:
        raise ValueError("temporal_block: h must be [b * frames * hw, C]")
    M, Cc = h.shape
    nq = 4 * ((3 * Cc // 4 + 31) // 32 * 32)
    if (not wqkv_frag.is_contiguous() or not wo_frag.is_contiguous() or wqkv_frag.numel() != nq * Cc or wo_frag.numel() != Cc * Cc
            or qkv_colsum.numel() != nq or qkv_bias.numel() != nq or tuple(posw.shape) != (frames, nq) or bo.numel() != Cc
            or not (qkv_colsum.is_contiguous() and qkv_bias.is_contiguous() and posw.is_contiguous() and bo.is_contiguous())):
        raise ValueError("temporal_block: wqkv_frag [nq / 32, C / 16, 64, 8] with qkv_colsum [nq], qkv_bias [nq], posw [frames, nq] "
                         "(nq = the regrouped, padded q|k|v columns); wo_frag [C / 32, C / 16, 64, 8] with bo [C]")
    if not stats.is_contiguous() or stats.dim() != 3 or stats.shape[0] != M or stats.shape[2] != 2:
        raise ValueError("temporal_block: stats must be contiguous f32 [M, C / 32 or 1, 2]")
    if rowstats is not None:
        _req(rowstats, F32, "rowstats")
        if not rowstats.is_contiguous() or tuple(rowstats.shape) != (M, Cc // 32, 2):
            raise ValueError("temporal_block: rowstats must be contiguous f32 [M, C / 32, 2]")
    if out is None:
        out = torch.empty((M, Cc), dtype=P.ACT, device=h.device)
    _req(out, P.ACT, "out")
    if out.shape != (M, Cc):
        raise ValueError("temporal_block: out must be [M, C]")
    if scale is None:
        scale = float(Cc // heads) ** -0.5
    a_ = (_p(h), _ld(h), _p(stats), int(stats.shape[1]), float(eps), _p(wqkv_frag), _p(qkv_colsum), _p(qkv_bias), _p(posw), _p(wo_frag),
          _p(bo), _p(out), _ld(out), _p(rowstats), b, frames, hw, Cc, heads, float(scale))
    _timed("temporal_block", 8.0 * M * Cc * Cc + 4.0 * M * frames * Cc, _nbytes(h, out, rowstats) + 2.0 * (nq + Cc) * Cc,
           (h, stats, wqkv_frag, qkv_colsum, qkv_bias, posw, wo_frag, bo, rowstats, out),
           lambda: check(_lib.lib().avsd_temporal_block(*a_, _stream()), "avsd_temporal_block"))
    return out


def temporal_attention(qkv: torch.Tensor, *, b: int, frames: int, hw: int, heads: int,
                       scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req(qkv, P.ACT, "qkv")
    Cc = qkv.shape[1] // 3
    d = Cc // heads
    if out is None:
        out = alloc16((qkv.shape[0], Cc), qkv.device)
    if scale is None:
        scale = float(d) ** -0.5
    if P.SPLIT:
        a_ = (_p(qkv), _ld(qkv), _lo(qkv), _p(out), _ld(out), _lo(out), b, frames, hw, heads, d, float(scale))
        call = lambda: check(_lib.lib().avsd_temporal_attention_x2(*a_, _stream()), "avsd_temporal_attention_x2")   # noqa: E731
    else:
        a_ = (_p(qkv), _ld(qkv), _p(out), _ld(out), b, frames, hw, heads, d, float(scale))
        call = lambda: check(_lib.lib().avsd_temporal_attention(*a_, _stream()), "avsd_temporal_attention")   # noqa: E731
    _timed("temporal_attention", 4.0 * b * hw * heads * frames * frames * d, _nbytes(qkv, out), (qkv, out), call)
    return out


def ncfhw_to_rows(x: torch.Tensor, cpad: int, rep: int = 1, scale: float = 1.0) -> torch.Tensor:
    _req(x, F32, "x")
    if not x.is_contiguous():
        raise ValueError("ncfhw_to_rows: x must be contiguous")
    B, Cc, Fr, H, W = x.shape
    out = alloc16((rep * B * Fr * H * W, cpad), x.device)
    if P.SPLIT:
        check(_lib.lib().avsd_ncfhw_to_rows_x2(_p(x), _p(out), _lo(out), B, Cc, Fr, H * W, cpad, rep, float(scale), _stream()),
              "avsd_ncfhw_to_rows_x2")
        return out
    check(_lib.lib().avsd_ncfhw_to_rows(_p(x), _p(out), B, Cc, Fr, H * W, cpad, rep, float(scale), _stream()),
          "avsd_ncfhw_to_rows")
    return out


def copy(src: torch.Tensor, dst: Optional[torch.Tensor] = None, rep: int = 1) -> torch.Tensor:
    """dst = `rep` copies of the contiguous tensor `src` along dim 0 (torch.cat([src] * rep)); with dst given, a device copy into
    it.  A library launch instead of a torch op, so that it is part of a recorded launch plan (asva_amd/plan.py)."""
    if not (src.is_cuda and src.is_contiguous()):
        raise ValueError("copy: src must be a contiguous device tensor")
    split = P.SPLIT and src.dtype == P.ACT          # a split tensor: both planes move
    if dst is None:
        shape = (rep * src.shape[0],) + tuple(src.shape[1:])
        dst = alloc16(shape, src.device) if split else torch.empty(shape, dtype=src.dtype, device=src.device)
    nbytes = src.numel() * src.element_size()
    if not dst.is_contiguous() or dst.numel() * dst.element_size() != rep * nbytes or nbytes % 16:
        raise ValueError("copy: dst must be contiguous and hold rep x src (a multiple of 16 bytes)")
    check(_lib.lib().avsd_copy(_p(src), _p(dst), nbytes, rep, _stream()), "avsd_copy")
    if split:
        check(_lib.lib().avsd_copy(_p(src) + 2 * _lo(src), _p(dst) + 2 * _lo(dst), nbytes, rep, _stream()), "avsd_copy")
    return dst


def xattn_pack_kv(kv: torch.Tensor, n_kv: int, rows: int, Cc: int, idx: Optional[torch.Tensor], k_out: torch.Tensor,
                  vt_out: torch.Tensor) -> None:
    """kv [n_kv*rows, 2C] -> k_out [nb, lk_pad, C], vt_out [nb, C, lk_pad] (operands of cross_attention_block); idx [F, nk]
    int32 gathers the visible keys of each frame (nb = n_kv * F).  The padding slots lk..lk_pad are zero-filled by the same launch."""
    _req(kv, P.ACT, "kv")
    _req(k_out, P.ACT, "k_out")
    _req(vt_out, P.ACT, "vt_out")
    if idx is not None:
        _req(idx, torch.int32, "idx")
    nfr, nk = (idx.shape if idx is not None else (0, 0))
    nb = n_kv * nfr if idx is not None else n_kv
    lkp = k_out.shape[1]
    if tuple(k_out.shape) != (nb, lkp, Cc) or tuple(vt_out.shape) != (nb, Cc, lkp) or not (kv.is_contiguous() and k_out.is_contiguous() and vt_out.is_contiguous()):
        raise ValueError("xattn_pack_kv: k_out [nb, lk_pad, C] / vt_out [nb, C, lk_pad] expected, all contiguous")
    check(_lib.lib().avsd_xattn_pack_kv(_p(kv), n_kv, rows, Cc, _p(idx), nfr, nk, _p(k_out), _p(vt_out), lkp, _stream()),
          "avsd_xattn_pack_kv")


def rows_to_ncfhw(rows: torch.Tensor, B: int, Cc: int, Fr: int, H: int, W: int) -> torch.Tensor:
    _req(rows, F32, "rows")
    out = torch.empty((B, Cc, Fr, H, W), dtype=F32, device=rows.device)
    check(_lib.lib().avsd_rows_to_ncfhw(_p(rows), _ld(rows), _p(out), B, Cc, Fr, H * W, _stream()), "avsd_rows_to_ncfhw")
    return out


def timestep_embedding(t: torch.Tensor, dim: int) -> torch.Tensor:
    _req(t, F32, "t")
    n = t.numel()
    out = torch.empty((n, dim), dtype=F32, device=t.device)
    check(_lib.lib().avsd_timestep_embedding(_p(t), _p(out), n, dim, _stream()), "avsd_timestep_embedding")
    return out


def _step_args(who: str, noise_pred, n_branch: int, xs, hist, store_slot: int, hist_idx, **weights):
    """What the three fused scheduler steps check and build alike.  `xs` = (x_in, x_out[, x_last]): contiguous f32 device tensors of
    one 5-d shape, noise_pred n_branch times that size; `hist` (slots, *x_in.shape) holds every ring slot named; one weight per
    hist_idx entry in each table.  -> (B, C, F, H * W), n_hist, the hist_idx table and the weight tables, padded to 4 entries"""
    names = ("x_in", "x_out", "x_last")[:len(xs)]
    for t, name in zip((noise_pred, *xs), ("noise_pred", *names)):
        _req(t, F32, name)
    x_in = xs[0]
    if (x_in.dim() != 5 or not all(t.is_contiguous() and t.shape == x_in.shape for t in xs) or not noise_pred.is_contiguous()
            or noise_pred.numel() != n_branch * x_in.numel()):
        raise ValueError(f"{who}: contiguous {' / '.join(names)} of one shape (B, C, F, H, W) and noise_pred of n_branch times their size")
    nh = len(hist_idx)
    if nh > 4 or any(len(w) != nh for w in weights.values()):
        raise ValueError(f"{who}: at most 4 history entries, with one {' and one '.join(weights)} weight each")
    slots = [s for s in (store_slot, *hist_idx) if s >= 0]
    if min(hist_idx, default=0) < 0 or (slots and (
            hist is None or not hist.is_contiguous() or hist.dtype != F32 or hist.device != x_in.device
            or tuple(hist.shape[1:]) != tuple(x_in.shape) or max(slots) >= hist.shape[0])):
        raise ValueError(f"{who}: slots {store_slot} / {tuple(hist_idx)} need hist_idx >= 0 and a contiguous f32 hist of shape "
                         f"(> {max(slots, default=0)}, {tuple(x_in.shape)}) on the latents' device")
    B, Cc, Fr, H, W = x_in.shape
    return ((B, Cc, Fr, H * W), nh, (C.c_int32 * 4)(*hist_idx, *[0] * (4 - nh)),
            [(C.c_float * 4)(*w, *[0.0] * (4 - nh)) for w in weights.values()])


def guided_step(noise_pred: torch.Tensor, n_branch: int, g: float, x_in: torch.Tensor, x_out: torch.Tensor,
                ca: float, cb: float, *, eps_hist: Optional[torch.Tensor] = None, store_slot: int = -1,
                w_cur: float = 1.0, hist_idx=(), w=(), g2: float = 0.0) -> None:
    """avsd_guided_step (include/avsd.h): one PLMS / DDIM step in place or out of place; `eps_hist` is (slots, *x_in.shape)."""
    (B, Cc, Fr, HW), nh, idx, (ws,) = _step_args("guided_step", noise_pred, n_branch, (x_in, x_out), eps_hist, store_slot, hist_idx, w=w)
    check(_lib.lib().avsd_guided_step(_p(noise_pred), n_branch, float(g), float(g2), _p(eps_hist), store_slot, float(w_cur), idx, ws,
                                      nh, _p(x_in), _p(x_out), float(ca), float(cb), B, Cc, Fr, HW, _stream()),
          "avsd_guided_step")


def guided_multistep(noise_pred: torch.Tensor, n_branch: int, g: float, x_in: torch.Tensor, x_out: torch.Tensor,
                     ca: float, c_cur: float, s_x: float, s_e: float, *, hist: Optional[torch.Tensor] = None, store_slot: int = -1,
                     hist_idx=(), w=(), g2: float = 0.0) -> None:
    """avsd_guided_multistep (include/avsd.h): one DPM-Solver++ step in place or out of place; `hist` is (slots, *x_in.shape)."""
    (B, Cc, Fr, HW), nh, idx, (ws,) = _step_args("guided_multistep", noise_pred, n_branch, (x_in, x_out), hist, store_slot, hist_idx, w=w)
    check(_lib.lib().avsd_guided_multistep(_p(noise_pred), n_branch, float(g), float(g2), _p(hist), store_slot, idx, ws, nh,
                                           _p(x_in), _p(x_out), float(ca), float(c_cur), float(s_x), float(s_e), B, Cc, Fr, HW,
                                           _stream()),
          "avsd_guided_multistep")


def _rng_ids(who: str, seed: int, stream: int, step: int):
    seed, stream, step = int(seed), int(stream), int(step)
    if not (0 <= seed < 1 << 64 and 0 <= stream < 1 << 32 and 0 <= step < 1 << 32):
        raise ValueError(f"{who}: seed is 64 bits and stream / step are 32 bits, all unsigned (seed={seed} stream={stream} step={step})")
    return seed, stream, step


def _noise_key(who: str, B: int, c_noise: float, seed: int, stream: int, step: int):
    """the trailing arguments of the two stochastic steps: batch row b draws from stream + b, which must stay a 32-bit id"""
    seed, stream, step = _rng_ids(who, seed, stream, step)
    if stream + B > 1 << 32:
        raise ValueError(f"{who}: stream + B exceeds 2^32 (stream={stream} B={B})")
    return float(c_noise), seed, stream, step


def guided_step_sde(noise_pred: torch.Tensor, n_branch: int, g: float, x_in: torch.Tensor, x_out: torch.Tensor,
                    ca: float, cb: float, *, eps_hist: Optional[torch.Tensor] = None, store_slot: int = -1,
                    w_cur: float = 1.0, hist_idx=(), w=(), g2: float = 0.0, c_noise: float = 0.0, seed: int = 0, stream: int = 0,
                    step: int = 0) -> None:
    """avsd_guided_step_sde (include/avsd.h): guided_step plus c_noise * z on frames 1.., z the normals of (seed, stream + b, step)
    in the layout (C, F - 1, H, W), evaluated inside the kernel."""
    (B, Cc, Fr, HW), nh, idx, (ws,) = _step_args("guided_step_sde", noise_pred, n_branch, (x_in, x_out), eps_hist, store_slot, hist_idx,
                                                 w=w)
    key = _noise_key("guided_step_sde", B, c_noise, seed, stream, step)
    check(_lib.lib().avsd_guided_step_sde(_p(noise_pred), n_branch, float(g), float(g2), _p(eps_hist), store_slot, float(w_cur), idx,
                                          ws, nh, _p(x_in), _p(x_out), float(ca), float(cb), B, Cc, Fr, HW, *key, _stream()),
          "avsd_guided_step_sde")


def guided_multistep_sde(noise_pred: torch.Tensor, n_branch: int, g: float, x_in: torch.Tensor, x_out: torch.Tensor,
                         ca: float, c_cur: float, s_x: float, s_e: float, *, hist: Optional[torch.Tensor] = None,
                         store_slot: int = -1, hist_idx=(), w=(), g2: float = 0.0, c_noise: float = 0.0, seed: int = 0,
                         stream: int = 0, step: int = 0) -> None:
    """avsd_guided_multistep_sde (include/avsd.h): guided_multistep plus c_noise * z on frames 1.., z as in guided_step_sde."""
    (B, Cc, Fr, HW), nh, idx, (ws,) = _step_args("guided_multistep_sde", noise_pred, n_branch, (x_in, x_out), hist, store_slot,
                                                 hist_idx, w=w)
    key = _noise_key("guided_multistep_sde", B, c_noise, seed, stream, step)
    check(_lib.lib().avsd_guided_multistep_sde(_p(noise_pred), n_branch, float(g), float(g2), _p(hist), store_slot, idx, ws, nh,
                                               _p(x_in), _p(x_out), float(ca), float(c_cur), float(s_x), float(s_e), B, Cc, Fr, HW,
                                               *key, _stream()),
          "avsd_guided_multistep_sde")


def _philox_fill(entry: str, dtype, n: int, seed: int, stream: int, step: int, first: int, device, out) -> torch.Tensor:
    n, first = int(n), int(first)
    seed, stream, step = _rng_ids(entry, seed, stream, step)
    if n < 0 or first < 0 or first + n >= 1 << 63:
        raise ValueError(f"{entry}: need n >= 0 and 0 <= first, first + n < 2^63 (n={n} first={first})")
    if out is None:
        out = torch.empty(n, dtype=dtype, device=device)
    _req(out, dtype, "out")
    if not out.is_contiguous() or out.numel() != n:
        raise ValueError(f"{entry}: out must be contiguous with {n} elements")
    if n:
        check(getattr(_lib.lib(), entry)(_p(out), n, seed, stream, step, first, _stream()), entry)
    return out


def philox_u32(n_words: int, seed: int, stream: int = 0, step: int = 0, first_word: int = 0, device="cuda",
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """avsd_philox4x32_u32 (include/avsd.h): words first_word .. first_word + n_words - 1 of the Philox4x32-10 sequence, as int32
    bit patterns (torch has no uint32 arithmetic; view the result as numpy uint32)."""
    return _philox_fill("avsd_philox4x32_u32", torch.int32, n_words, seed, stream, step, first_word, device, out)


def randn_philox(n: int, seed: int, stream: int = 0, step: int = 0, first: int = 0, device="cuda",
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """avsd_randn_philox_f32 (include/avsd.h): normals first .. first + n - 1 of the sequence (seed, stream, step), f32, flat; `out`
    (any shape, contiguous, n elements) is filled in place when given."""
    return _philox_fill("avsd_randn_philox_f32", F32, n, seed, stream, step, first, device, out)


def guided_unipc(noise_pred: torch.Tensor, n_branch: int, g: float, x_in: torch.Tensor, x_out: torch.Tensor, x_last: torch.Tensor,
                 use_corrector: bool, s_x: float, s_e: float, cc_last: float, cc_cur: float, cp_x: float, cp_cur: float, *,
                 hist: Optional[torch.Tensor] = None, store_slot: int = -1, hist_idx=(), wc=(), wp=(), g2: float = 0.0) -> None:
    """avsd_guided_unipc (include/avsd.h): one UniPC step (corrector of x_in from x_last, then predictor), x_out in place or out of
    place; `x_last` receives the corrected sample and aliases neither; `hist` is (slots, *x_in.shape)."""
    (B, Cc, Fr, HW), nh, idx, (wcs, wps) = _step_args("guided_unipc", noise_pred, n_branch, (x_in, x_out, x_last), hist, store_slot,
                                                      hist_idx, wc=wc, wp=wp)
    nbytes = x_in.numel() * 4
    if any(abs(x_last.data_ptr() - t.data_ptr()) < nbytes for t in (x_in, x_out)):
        raise ValueError("guided_unipc: x_last must not overlap x_in or x_out")
    check(_lib.lib().avsd_guided_unipc(_p(noise_pred), n_branch, float(g), float(g2), _p(hist), store_slot, idx, wcs, wps, nh,
                                       _p(x_in), _p(x_out), _p(x_last), int(bool(use_corrector)), float(s_x), float(s_e),
                                       float(cc_last), float(cc_cur), float(cp_x), float(cp_cur), B, Cc, Fr, HW, _stream()),
          "avsd_guided_unipc")


def window_turnover(x_prev: torch.Tensor, noise: torch.Tensor, x_next: Optional[torch.Tensor] = None, sigma: float = 1.0) -> torch.Tensor:
    """avsd_window_turnover (include/avsd.h): x_next[:, :, 0] = x_prev[:, :, F-1] bit-exact, x_next[:, :, 1:] = noise * sigma, one launch.
    x_prev, x_next (B, C, F, H, W) f32 contiguous, noise (B, C, F-1, H, W); x_next None or x_prev itself = in place."""
    _req(x_prev, F32, "x_prev")
    _req(noise, F32, "noise")
    x_next = x_prev if x_next is None else x_next
    _req(x_next, F32, "x_next")
    if x_prev.dim() != 5 or not (x_prev.is_contiguous() and x_next.is_contiguous() and noise.is_contiguous()) or x_next.shape != x_prev.shape:
        raise ValueError("window_turnover: contiguous x_prev / x_next of one shape (B, C, F, H, W)")
    B, Cc, Fr, H, W = x_prev.shape
    if tuple(noise.shape) != (B, Cc, Fr - 1, H, W) or not (x_next.device == x_prev.device == noise.device):
        raise ValueError(f"window_turnover: noise must be {(B, Cc, Fr - 1, H, W)} on the latents' device, got {tuple(noise.shape)}")
    nbytes = x_prev.numel() * 4
    if x_next.data_ptr() != x_prev.data_ptr() and abs(x_next.data_ptr() - x_prev.data_ptr()) < nbytes:
        raise ValueError("window_turnover: x_next must be x_prev itself or not overlap it")
    if noise.data_ptr() < x_next.data_ptr() + nbytes and x_next.data_ptr() < noise.data_ptr() + noise.numel() * 4:
        raise ValueError("window_turnover: noise must not overlap x_next")
    check(_lib.lib().avsd_window_turnover(_p(x_prev), _p(noise) if noise.numel() else None, _p(x_next), float(sigma), B, Cc, Fr, H * W,
                                          _stream()), "avsd_window_turnover")
    return x_next


FRAME_MSE_PARTS = 64     # AVSD_FRAME_MSE_PARTS (include/avsd.h): avsd_frame_mse_f32 wants B * FRAME_MSE_PARTS floats of scratch
DIFFUSE_MODES = {"epsilon": 0, "v": 1, "v_prediction": 1}


def _apart(a: torch.Tensor, b: torch.Tensor) -> bool:
    pa, pb = a.data_ptr(), b.data_ptr()
    return pa + a.numel() * a.element_size() <= pb or pb + b.numel() * b.element_size() <= pa


def check_timesteps(timesteps: torch.Tensor, n: int, T: int, device) -> torch.Tensor:
    """(n,) integer timesteps, all in [0, T) -> int32 vector on `device`.  Raises instead of clamping; a CPU tensor is checked on
    the host, a device tensor with one min / max read-back."""
    if timesteps.dim() != 1 or timesteps.numel() != n or timesteps.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"timesteps: expected an int32 / int64 vector of {n} entries, got {timesteps.dtype} {tuple(timesteps.shape)}")
    lo, hi = (int(v) for v in torch.aminmax(timesteps))
    if lo < 0 or hi >= T:
        raise ValueError(f"timesteps: [{lo}, {hi}] leaves the table's range [0, {T})")
    return timesteps.to(device=device, dtype=torch.int32).contiguous()


def diffuse_clip(x0: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor, sqrt_acp: torch.Tensor, sqrt_1m_acp: torch.Tensor,
                 keep_first: bool = True, mode: str = "epsilon", want_target: bool = True, noisy: Optional[torch.Tensor] = None,
                 target: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """avsd_diffuse_clip_f32 (include/avsd.h), one launch on contiguous (B, C, F, H, W) f32: noisy = a x0 + s noise with frame 0 kept
    bit-exact when keep_first, target = noise (epsilon) or a noise - s x0 (v).  -> (noisy, target); target is None unless wanted.
    timesteps: (B,) integers, validated against the tables' length here (ValueError), on any device."""
    if mode not in DIFFUSE_MODES:
        raise ValueError(f"diffuse_clip: mode must be one of {sorted(DIFFUSE_MODES)}, got {mode!r}")
    _req(x0, F32, "x0")
    _req(noise, F32, "noise")
    _req(sqrt_acp, F32, "sqrt_acp")
    _req(sqrt_1m_acp, F32, "sqrt_1m_acp")
    if x0.dim() != 5 or x0.numel() == 0 or noise.shape != x0.shape or not (x0.is_contiguous() and noise.is_contiguous()):
        raise ValueError("diffuse_clip: contiguous non-empty x0 / noise of one shape (B, C, F, H, W)")
    T = sqrt_acp.numel()
    if T == 0 or sqrt_acp.dim() != 1 or sqrt_1m_acp.shape != sqrt_acp.shape or not (sqrt_acp.device == sqrt_1m_acp.device == x0.device == noise.device):
        raise ValueError("diffuse_clip: two f32 tables of one length on the latents' device")
    B, Cc, Fr, H, W = x0.shape
    ts = check_timesteps(timesteps, B, T, x0.device)
    noisy = torch.empty_like(x0) if noisy is None else noisy
    if want_target and target is None:
        target = torch.empty_like(x0)
    outs = [noisy] + ([target] if target is not None else [])
    for o in outs:
        _req(o, F32, "output")
        if o.shape != x0.shape or not o.is_contiguous() or o.device != x0.device:
            raise ValueError("diffuse_clip: outputs must be contiguous with x0's shape on its device")
        if not all(_apart(o, i) for i in (x0, noise, ts, sqrt_acp, sqrt_1m_acp)):
            raise ValueError("diffuse_clip: an output overlaps an input (noisy may not be x0)")
    if target is not None and not _apart(noisy, target):
        raise ValueError("diffuse_clip: noisy and target overlap")
    check(_lib.lib().avsd_diffuse_clip_f32(_p(x0), _p(noise), _p(ts), _p(sqrt_acp), _p(sqrt_1m_acp), T, _p(noisy), _p(target),
                                           int(bool(keep_first)), DIFFUSE_MODES[mode], B, Cc, Fr, H * W, _stream()), "avsd_diffuse_clip_f32")
    return noisy, target


def frame_mse(pred: torch.Tensor, target: torch.Tensor, first_frame: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """avsd_frame_mse_f32 (include/avsd.h) on contiguous (B, C, F, H, W) f32 -> (loss 0-dim, per_sample (B,)): the mean squared
    difference over frames first_frame.. per sample, and its batch mean (= F.mse_loss of the sliced tensors).  Deterministic;
    per_sample[b] depends neither on B nor on b."""
    _req(pred, F32, "pred")
    _req(target, F32, "target")
    if pred.dim() != 5 or pred.numel() == 0 or target.shape != pred.shape or not (pred.is_contiguous() and target.is_contiguous()) or pred.device != target.device:
        raise ValueError("frame_mse: contiguous non-empty pred / target of one shape (B, C, F, H, W) on one device")
    B, Cc, Fr, H, W = pred.shape
    f0 = int(first_frame)
    if not 0 <= f0 < Fr:
        raise ValueError(f"frame_mse: no frames to score: first_frame {f0} of {Fr}")
    scratch = torch.empty((B * FRAME_MSE_PARTS + B + 1,), dtype=F32, device=pred.device)
    per_sample, loss = scratch[B * FRAME_MSE_PARTS:B * FRAME_MSE_PARTS + B], scratch[B * FRAME_MSE_PARTS + B:]
    check(_lib.lib().avsd_frame_mse_f32(_p(pred), _p(target), f0, _p(scratch), _p(per_sample), _p(loss), B, Cc, Fr, H * W, _stream()),
          "avsd_frame_mse_f32")
    return loss.reshape(()), per_sample


def vae_postprocess(rows: torch.Tensor, n_img: int, H: int, W: int) -> torch.Tensor:
    _req(rows, P.ACT, "rows")
    out = torch.empty((n_img, 3, H, W), dtype=F32, device=rows.device)
    if P.SPLIT:
        check(_lib.lib().avsd_vae_postprocess_x2(_p(rows), _ld(rows), _lo(rows), _p(out), n_img, H * W, _stream()), "avsd_vae_postprocess_x2")
        return out
    check(_lib.lib().avsd_vae_postprocess(_p(rows), _ld(rows), _p(out), n_img, H * W, _stream()), "avsd_vae_postprocess")
    return out


def vae_postprocess_u8(rows: torch.Tensor, n_img: int, H: int, W: int) -> torch.Tensor:
    _req(rows, P.ACT, "rows")
    out = torch.empty((n_img, H, W, 3), dtype=torch.uint8, device=rows.device)
    if P.SPLIT:
        check(_lib.lib().avsd_vae_postprocess_u8_x2(_p(rows), _ld(rows), _lo(rows), _p(out), n_img, H * W, _stream()),
              "avsd_vae_postprocess_u8_x2")
        return out
    check(_lib.lib().avsd_vae_postprocess_u8(_p(rows), _ld(rows), _p(out), n_img, H * W, _stream()), "avsd_vae_postprocess_u8")
    return out


# ---- audio conditioning front-end ------------------------------------------------------------------
def kaldi_fbank(wave: torch.Tensor, window: torch.Tensor, mel_fb: torch.Tensor, *, shift: int, nfft: int, t_out: int,
                preemph: float = 0.97, remove_dc: bool = True, mean: float = 0.0, std: float = 1.0) -> torch.Tensor:
    """wave (B, n_samples) f32 -> normalised log-mel (B, n_mel, t_out) f32; see avsd_kaldi_fbank."""
    _req(wave, F32, "wave")
    _req(window, F32, "window")
    _req(mel_fb, F32, "mel_fb")
    if wave.dim() != 2 or not mel_fb.is_contiguous() or mel_fb.shape[1] != nfft // 2 + 1:
        raise ValueError("kaldi_fbank: wave must be (B, n), mel_fb contiguous [n_mel][nfft/2+1]")
    B, n = wave.shape
    out = torch.empty((B, mel_fb.shape[0], t_out), dtype=F32, device=wave.device)
    check(_lib.lib().avsd_kaldi_fbank(_p(wave), B, n, wave.stride(0), _p(window), _p(mel_fb), window.numel(), shift, nfft,
                                      mel_fb.shape[0], float(preemph), int(remove_dc), _p(out), t_out, float(mean), float(std),
                                      _stream()), "avsd_kaldi_fbank")
    return out


# q (groups of `new` outputs that share one input window) per workgroup of avsd_resample_sinc_f32: 256 where that window fits
# 64 KiB of LDS, else 64 (csrc/audio.hip).  Tile boundaries sit at multiples of these times `orig` input samples.
RESAMPLE_QT = (64, 256)


def resample_sinc_f32(wave: torch.Tensor, taps: torch.Tensor, orig: int, new: int, width: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wave (n_wav, n_in) f32 -> (n_wav, ceil(new * n_in / orig)) f32 through the filter bank taps [new][2 * width + orig]
    (audio_features.resample_taps); see avsd_resample_sinc_f32.  Rows may be strided (views of a wider buffer); `out`, if
    given, is such a view to write into."""
    for name, t in (("wave", wave), ("taps", taps)) + ((("out", out),) if out is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"resample_sinc_f32: {name} must be a device tensor (libavsd_hip.so has no host path)")
        if t.dtype != F32:
            raise ValueError(f"resample_sinc_f32: {name} must be float32, got {t.dtype}")
    orig, new, width = int(orig), int(new), int(width)
    if orig <= 0 or new <= 0 or width <= 0:
        raise ValueError(f"resample_sinc_f32: orig, new, width must be positive, got {orig}, {new}, {width}")
    if wave.dim() != 2 or wave.shape[0] == 0 or wave.shape[1] == 0 or wave.stride(1) != 1:
        raise ValueError(f"resample_sinc_f32: wave must be a non-empty (n_wav, n_in) with unit inner stride, got {tuple(wave.shape)}")
    if tuple(taps.shape) != (new, 2 * width + orig) or not taps.is_contiguous():
        raise ValueError(f"resample_sinc_f32: taps must be contiguous [{new}][{2 * width + orig}], got {tuple(taps.shape)}")
    n_wav, n_in = wave.shape
    n_out = (new * n_in + orig - 1) // orig
    if out is None:
        out = torch.empty((n_wav, n_out), dtype=F32, device=wave.device)
    elif tuple(out.shape) != (n_wav, n_out) or out.stride(1) != 1 or out.device != wave.device:
        raise ValueError(f"resample_sinc_f32: out must be ({n_wav}, {n_out}) with unit inner stride on {wave.device}")
    check(_lib.lib().avsd_resample_sinc_f32(_p(wave), n_wav, n_in, wave.stride(0) if n_wav > 1 else max(wave.stride(0), n_in),
                                            _p(taps), orig, new, width, _p(out), n_out,
                                            out.stride(0) if n_wav > 1 else max(out.stride(0), n_out), _stream()),
          "avsd_resample_sinc_f32")
    return out


# ---- baseline JPEG encoder (csrc/jpeg.hip; host side in asva_amd/video_io.py) ------------------------------------------------
JPEG_SLOT_BYTES = 212      # AVSD_JPEG_SLOT_BYTES: the longest code string of one block, in whole 32-bit words


def jpeg_quantize(frames: torch.Tensor, qy: torch.Tensor, qc: torch.Tensor) -> torch.Tensor:
    """frames uint8 (n, H, W, 3) -> quantised DCT coefficients int16 (n, H/8, W/8, 3, 64) of Y, Cb, Cr in zigzag order; qy / qc:
    the 64 luminance / chrominance table entries in natural order as 16-bit integers on the device; see avsd_jpeg_quantize_u8."""
    for name, t, dt in (("frames", frames, (torch.uint8,)), ("qy", qy, (torch.int16, torch.uint16)), ("qc", qc, (torch.int16, torch.uint16))):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"jpeg_quantize: {name} must be a device tensor (libavsd_hip.so has no host path)")
        if t.dtype not in dt or not t.is_contiguous():
            raise ValueError(f"jpeg_quantize: {name} must be contiguous {dt[0]}, got {t.dtype}")
    if frames.dim() != 4 or frames.shape[-1] != 3 or frames.shape[0] == 0 or qy.numel() != 64 or qc.numel() != 64:
        raise ValueError(f"jpeg_quantize: frames must be a non-empty (n, H, W, 3) and the tables 64 entries, got {tuple(frames.shape)}, "
                         f"{qy.numel()}, {qc.numel()}")
    n, H, W, _ = frames.shape
    coef = torch.empty((n, H // 8, W // 8, 3, 64), dtype=torch.int16, device=frames.device)
    check(_lib.lib().avsd_jpeg_quantize_u8(_p(frames), n, H, W, _p(qy), _p(qc), _p(coef), _stream()), "avsd_jpeg_quantize_u8")
    return coef


def jpeg_pack(coef: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """coef int16 (n, ..., 64) with 3 x MCUs blocks per frame (what jpeg_quantize returns, or (n, blocks, 64)) -> (stream, nbytes):
    stream uint8 (n, blocks * 212), frame f's entropy-coded segment in stream[f, :nbytes[f]] (unstuffed, padded with 1-bits; the
    bytes behind it are not written), nbytes int32 (n,); see avsd_jpeg_pack_i16."""
    if not isinstance(coef, torch.Tensor) or not coef.is_cuda:
        raise ValueError("jpeg_pack: coef must be a device tensor (libavsd_hip.so has no host path)")
    if coef.dtype != torch.int16 or not coef.is_contiguous() or coef.dim() < 3 or coef.shape[-1] != 64 or coef.shape[0] == 0:
        raise ValueError(f"jpeg_pack: coef must be a non-empty contiguous int16 (n, ..., 64), got {coef.dtype} {tuple(coef.shape)}")
    n = coef.shape[0]
    blocks = coef.numel() // (n * 64)
    if blocks == 0 or blocks % 3:
        raise ValueError(f"jpeg_pack: {blocks} blocks per frame is not 3 x a number of MCUs")
    scratch = torch.empty((n * blocks * (JPEG_SLOT_BYTES + 8),), dtype=torch.uint8, device=coef.device)
    stream = torch.empty((n, blocks * JPEG_SLOT_BYTES), dtype=torch.uint8, device=coef.device)
    nbytes = torch.empty((n,), dtype=torch.int32, device=coef.device)
    check(_lib.lib().avsd_jpeg_pack_i16(_p(coef), n, blocks, _p(scratch), scratch.numel(), _p(stream), stream.stride(0), _p(nbytes),
                                        _stream()), "avsd_jpeg_pack_i16")
    return stream, nbytes


# ---- baseline JPEG decoder (csrc/jpeg.hip; host side in asva_amd/video_io.py) ------------------------------------------------
JPEG_HUFF_SET_WORDS = 6 * 352      # AVSD_JPEG_HUFF_SET_WORDS: [component][DC, AC] tables of 352 words
JPEG_SUBSEQ_BITS = 1024            # default length of a subsequence; any power of two in 128..4096 gives the same result
JPEG_SAMPLINGS = {"444": (0, 3, 8), "420": (1, 6, 16)}     # name -> (AVSD_JPEG_4xx, blocks per MCU, MCU edge in pixels)


def _jpeg_dev(name, t, dtypes, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{what}: {name} must be a device tensor (libavsd_hip.so has no host path)")
    if t.dtype not in dtypes or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous {dtypes[0]}, got {t.dtype}")


def jpeg_decode_scan(scan: torch.Tensor, offsets: torch.Tensor, nbits: torch.Tensor, table_index: torch.Tensor, tables: torch.Tensor,
                     blocks_per_frame: int, sampling: str, subseq_bits: int = JPEG_SUBSEQ_BITS, return_rounds: bool = False):
    """scan uint8 (bytes,): the frames' entropy-coded segments without stuffing, frame f at offsets[f] (int64, multiples of 4) with
    nbits[f] bits (int32) and at least 8 bytes of padding behind each; tables int32 (n_sets, 2112) as avsd.h describes them,
    table_index int32 (n,) -> (coef int16 (n, blocks_per_frame, 64) zigzag, DC absolute; status int32 (n,), 0 = decoded[; rounds
    int32 (n,)]).  See avsd_jpeg_decode_scan."""
    what = "jpeg_decode_scan"
    for name, t, dt in (("scan", scan, (torch.uint8,)), ("offsets", offsets, (torch.int64,)), ("nbits", nbits, (torch.int32,)),
                        ("table_index", table_index, (torch.int32,)), ("tables", tables, (torch.int32, torch.uint32))):
        _jpeg_dev(name, t, dt, what)
    if sampling not in JPEG_SAMPLINGS:
        raise ValueError(f"{what}: sampling must be one of {tuple(JPEG_SAMPLINGS)}, got {sampling!r}")
    n = offsets.numel()
    if n == 0 or nbits.numel() != n or table_index.numel() != n or tables.dim() != 2 or tables.shape[1] != JPEG_HUFF_SET_WORDS or scan.dim() != 1:
        raise ValueError(f"{what}: offsets, nbits and table_index need one entry per frame and tables {JPEG_HUFF_SET_WORDS} words per set, got "
                         f"{offsets.numel()}, {nbits.numel()}, {table_index.numel()}, {tuple(tables.shape)}")
    coef = torch.empty((n, blocks_per_frame, 64), dtype=torch.int16, device=scan.device)
    status = torch.empty((n,), dtype=torch.int32, device=scan.device)
    rounds = torch.empty((n,), dtype=torch.int32, device=scan.device) if return_rounds else None
    check(_lib.lib().avsd_jpeg_decode_scan(_p(scan), scan.numel(), _p(offsets), _p(nbits), _p(table_index), _p(tables), tables.shape[0], n,
                                           blocks_per_frame, JPEG_SAMPLINGS[sampling][0], subseq_bits, _p(coef), _p(status),
                                           _p(rounds) if return_rounds else None, _stream()), "avsd_jpeg_decode_scan")
    return (coef, status, rounds) if return_rounds else (coef, status)


def jpeg_idct_rgb(coef: torch.Tensor, H: int, W: int, sampling: str, qtabs: torch.Tensor, q_index: torch.Tensor) -> torch.Tensor:
    """coef int16 (n, blocks, 64) of n frames of H x W -> uint8 (n, H, W, 3); qtabs int16 (n_sets, 3, 64): each component's
    quantisation table in zigzag order, q_index int32 (n,).  See avsd_jpeg_idct_rgb_u8."""
    what = "jpeg_idct_rgb"
    for name, t, dt in (("coef", coef, (torch.int16,)), ("qtabs", qtabs, (torch.int16, torch.uint16)), ("q_index", q_index, (torch.int32,))):
        _jpeg_dev(name, t, dt, what)
    if sampling not in JPEG_SAMPLINGS:
        raise ValueError(f"{what}: sampling must be one of {tuple(JPEG_SAMPLINGS)}, got {sampling!r}")
    _, bpm, edge = JPEG_SAMPLINGS[sampling]
    mcus = -(-H // edge) * -(-W // edge)
    n = coef.shape[0]
    if coef.dim() != 3 or n == 0 or tuple(coef.shape[1:]) != (mcus * bpm, 64) or qtabs.dim() != 3 or tuple(qtabs.shape[1:]) != (3, 64) \
            or q_index.numel() != n:
        raise ValueError(f"{what}: {H} x {W} {sampling} needs coef (n, {mcus * bpm}, 64), qtabs (sets, 3, 64) and n table indices, got "
                         f"{tuple(coef.shape)}, {tuple(qtabs.shape)}, {q_index.numel()}")
    planes = torch.empty((n * mcus * 64 * (edge * edge // 64 + 2),), dtype=torch.uint8, device=coef.device)
    frames = torch.empty((n, H, W, 3), dtype=torch.uint8, device=coef.device)
    check(_lib.lib().avsd_jpeg_idct_rgb_u8(_p(coef), n, H, W, JPEG_SAMPLINGS[sampling][0], _p(qtabs), qtabs.shape[0], _p(q_index), _p(planes),
                                           planes.numel(), _p(frames), _stream()), "avsd_jpeg_idct_rgb_u8")
    return frames


def patchify(x: torch.Tensor, kh: int, kw: int, stride: int) -> torch.Tensor:
    """(B, C, H, W) f32 -> bf16 rows [B*ph*pw, C*kh*kw]."""
    _req(x, F32, "x")
    if not x.is_contiguous():
        raise ValueError("patchify: x must be contiguous")
    B, Cc, H, W = x.shape
    ph, pw = (H - kh) // stride + 1, (W - kw) // stride + 1
    if P.SPLIT:
        # split precision (once per clip, conditioning side): the gather is a strided device copy, the two planes come from
        # avsd_split_f32 — same values as the kernel's, with the rest plane kept
        cols = torch.nn.functional.unfold(x, (kh, kw), stride=stride)                 # (B, C*kh*kw, ph*pw), c-major then kh, kw
        return to_act(cols.transpose(1, 2).reshape(B * ph * pw, Cc * kh * kw))
    out = torch.empty((B * ph * pw, Cc * kh * kw), dtype=P.ACT, device=x.device)
    check(_lib.lib().avsd_patchify(_p(x), _p(out), B, Cc, H, W, kh, kw, stride, _stream()), "avsd_patchify")
    return out


def vit_tokens(patches: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, b: int, tail_rows: int = 0) -> torch.Tensor:
    """bf16 patch embeddings [b*np, C] + cls [C] + pos [1+np, C] (f32) -> bf16 [b*(1+np+tail_rows), C]."""
    _req(patches, P.ACT, "patches")
    _req(cls, F32, "cls")
    _req(pos, F32, "pos")
    n_p, Cc = patches.shape[0] // b, patches.shape[1]
    if not patches.is_contiguous() or pos.shape != (1 + n_p, Cc) or cls.numel() != Cc:
        raise ValueError("vit_tokens: shape mismatch")
    if P.SPLIT:          # split precision: the same f32 sums, both planes (device ops + avsd_split_f32; once per clip)
        tok = torch.zeros((b, 1 + n_p + tail_rows, Cc), dtype=F32, device=patches.device)
        tok[:, 0] = cls.reshape(1, Cc) + pos[0]
        tok[:, 1:1 + n_p] = from_act(patches).view(b, n_p, Cc) + pos[1:]
        return to_act(tok.view(-1, Cc))
    out = torch.empty((b * (1 + n_p + tail_rows), Cc), dtype=P.ACT, device=patches.device)
    check(_lib.lib().avsd_vit_tokens(_p(patches), _p(cls), _p(pos), _p(out), b, n_p, Cc, tail_rows, _stream()), "avsd_vit_tokens")
    return out


# ---- AVSync scorer (csrc/avsync.hip): f32 tensors, channels-last, the same arithmetic in both builds of the library -----------
def convnd_f32(x: torch.Tensor, w: torch.Tensor, taps, stride, pad, *, bias: Optional[torch.Tensor] = None,
               res: Optional[torch.Tensor] = None, rscale: Optional[torch.Tensor] = None, relu: bool = False,
               w_col: int = 0) -> torch.Tensor:
    """x [n, t, h, w, cin], w [cout, ldw >= taps * cin] (tap-major, cin-minor) -> act(conv + bias + rscale * res) [n, to, ho, wo, cout];
    see avsd_convnd_f32.  w_col > 0: the weight is the column block w[:, w_col:w_col + taps * cin] of the packed matrix (ldw stays
    its row stride) — one half of a layer that is linear in a concatenation."""
    for t, name in ((x, "x"), (w, "w"), (bias, "bias"), (res, "res"), (rscale, "rscale")):
        if t is not None and (t.dtype != F32 or not t.is_cuda or not t.is_contiguous()):   # (a size-1 channel axis may carry any stride)
            raise ValueError(f"convnd_f32: {name} must be a contiguous f32 device tensor")
    if x.dim() != 5 or w.dim() != 2:
        raise ValueError("convnd_f32: x must be [n, t, h, w, cin], w [cout, ldw]")
    n, ti, hi, wi, cin = x.shape
    cout, ldw = w.shape
    (kt, kh, kw), (st, sh, sw), (pt, ph, pw) = taps, stride, pad
    to, ho, wo = (ti + 2 * pt - kt) // st + 1, (hi + 2 * ph - kh) // sh + 1, (wi + 2 * pw - kw) // sw + 1
    if min(to, ho, wo) < 1:
        raise ValueError(f"convnd_f32: input {(ti, hi, wi)} is smaller than the window {tuple(taps)}")
    if res is not None and tuple(res.shape) != (n, to, ho, wo, cout):
        raise ValueError(f"convnd_f32: residual {tuple(res.shape)} does not match the output {(n, to, ho, wo, cout)}")
    if any(v is not None and v.numel() != cout for v in (bias, rscale)):
        raise ValueError("convnd_f32: bias / rscale must have cout entries")
    w_col = int(w_col)
    # (w_col == 0 is every earlier call: a row shorter than K stays the library's refusal, with its message)
    if w_col < 0 or (w_col > 0 and w_col + kt * kh * kw * cin > ldw):
        raise ValueError(f"convnd_f32: columns {w_col} .. {w_col + kt * kh * kw * cin} leave the weight rows of {ldw} floats")
    out = torch.empty((n, to, ho, wo, cout), dtype=F32, device=x.device)
    check(_lib.lib().avsd_convnd_f32(_p(x), _p(w) + 4 * w_col, _p(bias), _p(res), _p(rscale), _p(out), n, ti, hi, wi, cin, to, ho, wo, cout,
                                     kt, kh, kw, st, sh, sw, pt, ph, pw, ldw, int(relu), _stream()), "avsd_convnd_f32")
    return out


def linear_f32(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [m, K], w [N, ldw >= K] -> x @ w[:, :K].T + b + res, [m, N]: convnd_f32 with a (1, 1, 1) window over m images of 1 x 1 x 1"""
    m = x.shape[0]
    r = None if res is None else res.view(m, 1, 1, 1, -1)
    return convnd_f32(x.view(m, 1, 1, 1, -1), w, (1, 1, 1), (1, 1, 1), (0, 0, 0), bias=b, res=r).view(m, -1)


def pair_head_supported(D: int, H1: int, H2: int) -> bool:
    """the head sizes avsd_pair_head_f32 is built for (the real head: 512 / 512 / 256)"""
    return D % 32 == 0 and H1 % 32 == 0 and H2 % 32 == 0 and 0 < H2 <= 256 and D > 0 and H1 > 0


def pair_head_f32(u: torch.Tensor, vh: torch.Tensor, w2: torch.Tensor, b2: Optional[torch.Tensor], w3: torch.Tensor,
                  b3: Optional[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """avsd_pair_head_f32 (include/avsd.h): u [G, P, H1], vh [G, Q, H1], w2 [H2, ldw2 >= H1], b2 [H2], w3 [>= 1, ldw3 >= H2] (row 0 is
    read), b3 [>= 1] -> scores [G, P, Q], one launch.  `out`: a contiguous f32 [G, P, Q] device tensor to write into."""
    for t, name in ((u, "u"), (vh, "vh"), (w2, "w2"), (b2, "b2"), (w3, "w3"), (b3, "b3"), (out, "out")):
        if t is not None and (t.dtype != F32 or not t.is_cuda or not t.is_contiguous()):
            raise ValueError(f"pair_head_f32: {name} must be a contiguous f32 device tensor")
    if u.dim() != 3 or vh.dim() != 3 or u.shape[0] != vh.shape[0] or u.shape[2] != vh.shape[2] or u.numel() == 0 or vh.numel() == 0:
        raise ValueError(f"pair_head_f32: u must be [G, P, H1] and vh [G, Q, H1], got {tuple(u.shape)} and {tuple(vh.shape)}")
    (G, Pn, H1), Q = u.shape, vh.shape[1]
    if w2.dim() != 2 or w2.shape[1] < H1 or w3.dim() != 2 or w3.shape[1] < w2.shape[0]:
        raise ValueError(f"pair_head_f32: w2 must be [H2, >= {H1}] and w3 [out_dim, >= H2], got {tuple(w2.shape)} and {tuple(w3.shape)}")
    H2, ldw2 = w2.shape
    if (b2 is not None and b2.numel() != H2) or (b3 is not None and b3.numel() < 1):
        raise ValueError("pair_head_f32: b2 must have H2 entries and b3 at least one")
    if out is None:
        out = torch.empty((G, Pn, Q), dtype=F32, device=u.device)
    elif tuple(out.shape) != (G, Pn, Q) or out.device != u.device:
        raise ValueError(f"pair_head_f32: out must be {(G, Pn, Q)} on the inputs' device")
    check(_lib.lib().avsd_pair_head_f32(_p(u), _p(vh), _p(w2), ldw2, _p(b2), _p(w3), _p(b3), _p(out), G, Pn, Q, H1, H2, _stream()),
          "avsd_pair_head_f32")
    return out


def pair_xent_f32(scores: torch.Tensor, tau: float = 1.0) -> dict:
    """avsd_pair_xent_f32 (include/avsd.h) on contiguous scores [G, P, Q] -> dict(row_argmax [G, P] int32, col_argmax [G, Q] int32,
    row_loss [G, P] when P <= Q, col_loss [G, Q] when Q <= P, and when P == Q av_loss, va_loss, av_acc, va_acc as 0-d f32)."""
    _req(scores, F32, "scores")
    if scores.dim() != 3 or scores.numel() == 0 or not scores.is_contiguous():
        raise ValueError(f"pair_xent_f32: scores must be a contiguous non-empty [G, P, Q], got {tuple(scores.shape)}")
    tau = float(tau)
    if not (tau > 0.0 and tau < float("inf")):
        raise ValueError(f"pair_xent_f32: tau must be positive and finite, got {tau}")
    G, Pn, Q = scores.shape
    dev = scores.device
    r = {"row_argmax": torch.empty((G, Pn), dtype=torch.int32, device=dev), "col_argmax": torch.empty((G, Q), dtype=torch.int32, device=dev)}
    if Pn <= Q:
        r["row_loss"] = torch.empty((G, Pn), dtype=F32, device=dev)
    if Q <= Pn:
        r["col_loss"] = torch.empty((G, Q), dtype=F32, device=dev)
    means = torch.empty((4,), dtype=F32, device=dev) if Pn == Q else None
    check(_lib.lib().avsd_pair_xent_f32(_p(scores), 1.0 / tau, _p(r.get("row_loss")), _p(r.get("col_loss")), _p(r["row_argmax"]),
                                        _p(r["col_argmax"]), _p(means), G, Pn, Q, _stream()), "avsd_pair_xent_f32")
    if means is not None:
        r.update(av_loss=means[0], va_loss=means[1], av_acc=means[2], va_acc=means[3])
    return r


def maxpool_hw_f32(x: torch.Tensor) -> torch.Tensor:
    """[n, t, h, w, c] -> [n, t, ho, wo, c]: (1, 3, 3) window, stride (1, 2, 2), padding (0, 1, 1)"""
    _req(x, F32, "x")
    if x.dim() != 5 or not x.is_contiguous():
        raise ValueError("maxpool_hw_f32: x must be contiguous [n, t, h, w, c]")
    n, t, hi, wi, c = x.shape
    ho, wo = (hi - 1) // 2 + 1, (wi - 1) // 2 + 1
    out = torch.empty((n, t, ho, wo, c), dtype=F32, device=x.device)
    check(_lib.lib().avsd_maxpool_hw_f32(_p(x), _p(out), n * t, hi, wi, c, ho, wo, _stream()), "avsd_maxpool_hw_f32")
    return out


def _slice_ld(t: torch.Tensor, name: str) -> int:
    """t [n, a, h, w, c]: a channel slice of a contiguous channels-last buffer [n, a, h, w, ld] (or the whole of it); -> ld"""
    if t.dtype != F32 or not t.is_cuda or t.dim() != 5:
        raise ValueError(f"{name} must be a 5-d f32 device tensor [n, t, h, w, c]")
    n, a, h, w, c = t.shape
    ld = t.stride(3) if n * a * h * w > 1 else max(t.stride(3), c)
    want = (a * h * w * ld, h * w * ld, w * ld, ld, 1)
    if ld < c or any(t.shape[i] > 1 and t.stride(i) != want[i] for i in range(5)):
        raise ValueError(f"{name} {tuple(t.shape)} with strides {tuple(t.stride())} is not a channel slice of a contiguous channels-last buffer")
    return ld


def convnd_ld_f32(x: torch.Tensor, w: torch.Tensor, taps, stride, pad, *, out: Optional[torch.Tensor] = None,
                  bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, rscale: Optional[torch.Tensor] = None,
                  relu: bool = False, ldx: Optional[int] = None, ldy: Optional[int] = None) -> torch.Tensor:
    """convnd_f32 on channel slices: x [n, t, h, w, cin] may be a view x_wide[..., a:a + cin] of a contiguous channels-last buffer, and
    `out`, if given, a view out_wide[..., b:b + cout] that the result is written into (columns outside it are not touched).  `res` has
    the shape and the pixel stride of out.  ldx / ldy, if given, replace the pixel strides read from the views by smaller ones; see
    avsd_convnd_ld_f32"""
    for t, name in ((w, "w"), (bias, "bias"), (rscale, "rscale")):
        if t is not None and (t.dtype != F32 or not t.is_cuda or not t.is_contiguous()):
            raise ValueError(f"convnd_ld_f32: {name} must be a contiguous f32 device tensor")
    if w.dim() != 2:
        raise ValueError("convnd_ld_f32: w must be [cout, ldw]")
    sx = _slice_ld(x, "convnd_ld_f32: x")
    if ldx is not None and ldx > sx:
        raise ValueError(f"convnd_ld_f32: ldx {ldx} is wider than the pixel stride {sx} of x")
    ldx = sx if ldx is None else int(ldx)
    n, ti, hi, wi, cin = x.shape
    cout, ldw = w.shape
    (kt, kh, kw), (st, sh, sw), (pt, ph, pw) = taps, stride, pad
    to, ho, wo = (ti + 2 * pt - kt) // st + 1, (hi + 2 * ph - kh) // sh + 1, (wi + 2 * pw - kw) // sw + 1
    if min(to, ho, wo) < 1:
        raise ValueError(f"convnd_ld_f32: input {(ti, hi, wi)} is smaller than the window {tuple(taps)}")
    if any(v is not None and v.numel() != cout for v in (bias, rscale)):
        raise ValueError("convnd_ld_f32: bias / rscale must have cout entries")
    if out is None:
        out = torch.empty((n, to, ho, wo, cout), dtype=F32, device=x.device)
    elif tuple(out.shape) != (n, to, ho, wo, cout):
        raise ValueError(f"convnd_ld_f32: out {tuple(out.shape)} does not match {(n, to, ho, wo, cout)}")
    sy = _slice_ld(out, "convnd_ld_f32: out")
    if ldy is not None and ldy > sy:
        raise ValueError(f"convnd_ld_f32: ldy {ldy} is wider than the pixel stride {sy} of out")
    ldy = sy if ldy is None else int(ldy)
    if res is not None and (tuple(res.shape) != tuple(out.shape) or _slice_ld(res, "convnd_ld_f32: res") != sy):
        raise ValueError(f"convnd_ld_f32: res must have the shape {tuple(out.shape)} and the pixel stride {sy} of out")
    check(_lib.lib().avsd_convnd_ld_f32(_p(x), ldx, _p(w), _p(bias), _p(res), _p(rscale), _p(out), ldy, n, ti, hi, wi, cin, to, ho, wo, cout,
                                        kt, kh, kw, st, sh, sw, pt, ph, pw, ldw, int(relu), _stream()), "avsd_convnd_ld_f32")
    return out


def pool3_hw_f32(x: torch.Tensor, mode: str, stride: int, pad: int, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3 x 3 pool on [n, t, h, w, c] (each of the n * t images on its own), mode "max" or "avg" (padded positions not counted),
    (stride, pad) = (2, 0) or (1, 1); x and `out` may be channel slices as in convnd_ld_f32; see avsd_pool3_hw_f32"""
    if mode not in ("max", "avg"):
        raise ValueError(f"pool3_hw_f32: mode {mode!r}")
    ldx = _slice_ld(x, "pool3_hw_f32: x")
    n, t, hi, wi, c = x.shape
    ho, wo = (hi + 2 * pad - 3) // stride + 1, (wi + 2 * pad - 3) // stride + 1
    if min(ho, wo) < 1:
        raise ValueError(f"pool3_hw_f32: input {(hi, wi)} is smaller than the window")
    if out is None:
        out = torch.empty((n, t, ho, wo, c), dtype=F32, device=x.device)
    elif tuple(out.shape) != (n, t, ho, wo, c):
        raise ValueError(f"pool3_hw_f32: out {tuple(out.shape)} does not match {(n, t, ho, wo, c)}")
    ldy = _slice_ld(out, "pool3_hw_f32: out")
    check(_lib.lib().avsd_pool3_hw_f32(_p(x), ldx, _p(out), ldy, n * t, hi, wi, c, ho, wo, int(stride), int(pad), int(mode == "avg"),
                                       _stream()), "avsd_pool3_hw_f32")
    return out


def same_pad(size: int, k: int, s: int):
    """TensorFlow "same" padding of one axis -> (front, back); the output is ceil(size / s) (pytorch_i3d.py:73-95)"""
    total = max(k - (s if size % s == 0 else size % s), 0)
    return total // 2, total - total // 2


def conv3d_same_f32(x: torch.Tensor, w: torch.Tensor, taps, stride, *, out: Optional[torch.Tensor] = None,
                    bias: Optional[torch.Tensor] = None, relu: bool = False, loader: int = 0, ldx: Optional[int] = None,
                    ldy: Optional[int] = None) -> torch.Tensor:
    """convnd_ld_f32 with "same" zero padding computed from the input size: x [n, t, h, w, cin] (a channel slice or dense) ->
    [n, ceil(t / st), ceil(h / sh), ceil(w / sw), cout], into the channel slice `out` if given.  loader 0 picks; 1 / 2 / 3 force the
    scalar / float4 / run loader (same bits; refused where illegal); see avsd_conv3d_same_f32"""
    for t, name in ((w, "w"), (bias, "bias")):
        if t is not None and (t.dtype != F32 or not t.is_cuda or not t.is_contiguous()):
            raise ValueError(f"conv3d_same_f32: {name} must be a contiguous f32 device tensor")
    if w.dim() != 2:
        raise ValueError("conv3d_same_f32: w must be [cout, ldw]")
    sx = _slice_ld(x, "conv3d_same_f32: x")
    if ldx is not None and ldx > sx:
        raise ValueError(f"conv3d_same_f32: ldx {ldx} is wider than the pixel stride {sx} of x")
    ldx = sx if ldx is None else int(ldx)
    n, ti, hi, wi, cin = x.shape
    cout, ldw = w.shape
    (kt, kh, kw), (st, sh, sw) = taps, stride
    if min(st, sh, sw) < 1:
        raise ValueError("conv3d_same_f32: strides must be positive")
    to, ho, wo = -(-ti // st), -(-hi // sh), -(-wi // sw)
    if bias is not None and bias.numel() != cout:
        raise ValueError("conv3d_same_f32: bias must have cout entries")
    if out is None:
        out = torch.empty((n, to, ho, wo, cout), dtype=F32, device=x.device)
    elif tuple(out.shape) != (n, to, ho, wo, cout):
        raise ValueError(f"conv3d_same_f32: out {tuple(out.shape)} does not match {(n, to, ho, wo, cout)}")
    sy = _slice_ld(out, "conv3d_same_f32: out")
    if ldy is not None and ldy > sy:
        raise ValueError(f"conv3d_same_f32: ldy {ldy} is wider than the pixel stride {sy} of out")
    ldy = sy if ldy is None else int(ldy)
    check(_lib.lib().avsd_conv3d_same_f32(_p(x), ldx, _p(w), _p(bias), _p(out), ldy, n, ti, hi, wi, cin, to, ho, wo, cout, kt, kh, kw, st, sh,
                                          sw, ldw, int(relu), int(loader), _stream()), "avsd_conv3d_same_f32")
    return out


def maxpool3d_same_f32(x: torch.Tensor, window, stride, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """max pool with "same" padding on [n, t, h, w, c], windows 1 .. 3 and strides 1 .. 2 per axis; a padded position counts as 0.0;
    x and `out` may be channel slices as in convnd_ld_f32; see avsd_maxpool3d_same_f32"""
    ldx = _slice_ld(x, "maxpool3d_same_f32: x")
    n, ti, hi, wi, c = x.shape
    (kt, kh, kw), (st, sh, sw) = window, stride
    if min(st, sh, sw) < 1:
        raise ValueError("maxpool3d_same_f32: strides must be positive")
    to, ho, wo = -(-ti // st), -(-hi // sh), -(-wi // sw)
    if out is None:
        out = torch.empty((n, to, ho, wo, c), dtype=F32, device=x.device)
    elif tuple(out.shape) != (n, to, ho, wo, c):
        raise ValueError(f"maxpool3d_same_f32: out {tuple(out.shape)} does not match {(n, to, ho, wo, c)}")
    ldy = _slice_ld(out, "maxpool3d_same_f32: out")
    check(_lib.lib().avsd_maxpool3d_same_f32(_p(x), ldx, _p(out), ldy, n, ti, hi, wi, c, to, ho, wo, kt, kh, kw, st, sh, sw, _stream()),
          "avsd_maxpool3d_same_f32")
    return out


def mean_rows_f32(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n, ..., c] -> [n, c]: mean over all positions of a sample, into the contiguous `out` [n, c] if given"""
    _req(x, F32, "x")
    if x.dim() < 2 or not x.is_contiguous():
        raise ValueError("mean_rows_f32: x must be contiguous [n, ..., c]")
    n, c = x.shape[0], x.shape[-1]
    if out is None:
        out = torch.empty((n, c), dtype=F32, device=x.device)
    elif out.dtype != F32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (n, c):
        raise ValueError(f"mean_rows_f32: out must be a contiguous f32 device tensor {(n, c)}")
    check(_lib.lib().avsd_mean_rows_f32(_p(x), _p(out), n, x.numel() // (n * c), c, _stream()), "avsd_mean_rows_f32")
    return out


def resize_aa_normalize_f32(frames: torch.Tensor, ytab, xtab, size: int, crop: int, mean, std) -> torch.Tensor:
    """frames (n, 3, H, W) f32 -> [n, size, size, 3] resized with the host-built taps ytab / xtab = (start i32 [size], count i32 [size],
    weight f32 [size, taps]) and normalised per channel; see avsd_resize_aa_normalize_f32"""
    _req(frames, F32, "frames")
    if frames.dim() != 4 or frames.shape[1] != 3 or not frames.is_contiguous():
        raise ValueError("resize_aa_normalize_f32: frames must be contiguous (n, 3, H, W)")
    n, _, hi, wi = frames.shape
    for (s, cnt, wt), name in ((ytab, "ytab"), (xtab, "xtab")):
        _req(wt, F32, name)
        if s.dtype != torch.int32 or cnt.dtype != torch.int32 or s.numel() != size or cnt.numel() != size or wt.shape[0] != size \
                or not (s.is_cuda and cnt.is_cuda and wt.is_contiguous()):
            raise ValueError(f"resize_aa_normalize_f32: {name} must be (int32 [size], int32 [size], f32 [size, taps]) on the device")
    tmp = torch.empty((n, 3, hi, size), dtype=F32, device=frames.device)
    out = torch.empty((n, size, size, 3), dtype=F32, device=frames.device)
    check(_lib.lib().avsd_resize_aa_normalize_f32(_p(frames), _p(tmp), _p(out), n, hi, wi, size, size, _p(ytab[0]), _p(ytab[1]), _p(ytab[2]),
                                                  ytab[2].shape[1], _p(xtab[0]), _p(xtab[1]), _p(xtab[2]), xtab[2].shape[1], crop,
                                                  *[float(v) for v in mean], *[float(v) for v in std], _stream()),
          "avsd_resize_aa_normalize_f32")
    return out


# ---- CLIP text encoder (csrc/clip_text.hip): f32 tensors, the same arithmetic in both builds of the library --------------------
def embed_tokens_f32(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, b: int, seq: int) -> torch.Tensor:
    """ids int32 [b * seq] (already checked against the table size on the host), tok [V, C], pos [>= seq, C] -> tok[ids] + pos, [b * seq, C]"""
    _req(tok, F32, "tok")
    _req(pos, F32, "pos")
    if ids.dtype != torch.int32 or not ids.is_cuda or not ids.is_contiguous() or ids.numel() != b * seq:
        raise ValueError("embed_tokens_f32: ids must be a contiguous int32 device tensor of b * seq entries")
    if tok.dim() != 2 or pos.dim() != 2 or not tok.is_contiguous() or not pos.is_contiguous() or pos.shape[1] != tok.shape[1] or pos.shape[0] < seq:
        raise ValueError("embed_tokens_f32: tok must be contiguous [V, C], pos contiguous [>= seq, C]")
    v, c = tok.shape
    out = torch.empty((b * seq, c), dtype=F32, device=tok.device)
    check(_lib.lib().avsd_embed_tokens_f32(_p(ids), _p(tok), _p(pos), _p(out), b, seq, c, v, _stream()), "avsd_embed_tokens_f32")
    return out


def layernorm_f32(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [M, C] f32 (rows may be a column slice of a wider buffer) -> LayerNorm over C, [M, C]; `out` may be x"""
    _req(x, F32, "x")
    _req(gamma, F32, "gamma")
    _req(beta, F32, "beta")
    if x.dim() != 2 or gamma.numel() != x.shape[1] or beta.numel() != x.shape[1] or not gamma.is_contiguous() or not beta.is_contiguous():
        raise ValueError("layernorm_f32: x must be [M, C], gamma and beta contiguous [C]")
    m, c = x.shape
    if out is None:
        out = torch.empty((m, c), dtype=F32, device=x.device)
    else:
        _req(out, F32, "out")
        if tuple(out.shape) != (m, c):
            raise ValueError("layernorm_f32: out must have the shape of x")
    ldx, ldy = (x.stride(0) if m > 1 else c), (out.stride(0) if m > 1 else c)
    check(_lib.lib().avsd_layernorm_f32(_p(x), ldx, _p(out), ldy, m, c, _p(gamma), _p(beta), float(eps), _stream()), "avsd_layernorm_f32")
    return out


def attention_causal_f32(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, b: int, seq: int, heads: int,
                         scale: Optional[float] = None) -> torch.Tensor:
    """q, k, v [b * seq, heads * d] f32 (usually column slices of one fused [b * seq, 3 C] buffer) -> causal self-attention within each of
    the b sequences, [b * seq, heads * d]; see avsd_attention_causal_f32"""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        _req(t, F32, name)
        if t.dim() != 2 or tuple(t.shape) != tuple(q.shape) or t.shape[0] != b * seq or t.shape[1] % heads:
            raise ValueError(f"attention_causal_f32: {name} must be [b * seq, heads * d]")
    c = q.shape[1]
    d = c // heads
    ld = [t.stride(0) if b * seq > 1 else c for t in (q, k, v)]
    out = torch.empty((b * seq, c), dtype=F32, device=q.device)
    check(_lib.lib().avsd_attention_causal_f32(_p(q), ld[0], _p(k), ld[1], _p(v), ld[2], _p(out), c, b, seq, heads, d,
                                               float(d ** -0.5 if scale is None else scale), _stream()), "avsd_attention_causal_f32")
    return out


def quick_gelu_f32(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x * sigmoid(1.702 x) elementwise on a contiguous f32 tensor; `out` may be x"""
    _req(x, F32, "x")
    out = torch.empty_like(x) if out is None else out
    _req(out, F32, "out")
    if not x.is_contiguous() or not out.is_contiguous() or out.numel() != x.numel():
        raise ValueError("quick_gelu_f32: x and out must be contiguous and of one size")
    check(_lib.lib().avsd_quick_gelu_f32(_p(x), _p(out), x.numel(), _stream()), "avsd_quick_gelu_f32")
    return out


# ---- ImageBind evaluation towers (csrc/imagebind_eval.hip): f32 tensors, the same arithmetic in both builds of the library --------
def attention_f32(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, b: int, seq: int, heads: int, scale: Optional[float] = None) -> torch.Tensor:
    """q, k, v [b * seq, heads * d] f32 (usually column slices of one fused [b * seq, 3 C] buffer) -> bidirectional self-attention within
    each of the b sequences, [b * seq, heads * d]; d is 64 or 80; see avsd_attention_f32"""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        _req(t, F32, name)
        if t.dim() != 2 or tuple(t.shape) != tuple(q.shape) or t.shape[0] != b * seq or t.shape[1] % heads:
            raise ValueError(f"attention_f32: {name} must be [b * seq, heads * d]")
    c = q.shape[1]
    d = c // heads
    ld = [t.stride(0) if b * seq > 1 else c for t in (q, k, v)]
    out = torch.empty((b * seq, c), dtype=F32, device=q.device)
    check(_lib.lib().avsd_attention_f32(_p(q), ld[0], _p(k), ld[1], _p(v), ld[2], _p(out), c, b, seq, heads, d,
                                        float(d ** -0.5 if scale is None else scale), _stream()), "avsd_attention_f32")
    return out


def gelu_f32(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """0.5 x (1 + erf(x / sqrt 2)) elementwise on a contiguous f32 tensor; `out` may be x"""
    _req(x, F32, "x")
    out = torch.empty_like(x) if out is None else out
    _req(out, F32, "out")
    if not x.is_contiguous() or not out.is_contiguous() or out.numel() != x.numel():
        raise ValueError("gelu_f32: x and out must be contiguous and of one size")
    check(_lib.lib().avsd_gelu_f32(_p(x), _p(out), x.numel(), _stream()), "avsd_gelu_f32")
    return out


def vit_tokens_f32(patches: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, b: int, tail_rows: int = 0) -> torch.Tensor:
    """f32 patch embeddings [b * np, C] + cls [C] + pos [1 + np, C] -> f32 [b * (1 + np + tail_rows), C] with zero tail rows"""
    _req(patches, F32, "patches")
    _req(cls, F32, "cls")
    _req(pos, F32, "pos")
    if patches.dim() != 2 or b < 1 or patches.shape[0] % b:
        raise ValueError("vit_tokens_f32: patches must be [b * np, C]")
    n_p, c = patches.shape[0] // b, patches.shape[1]
    if not (patches.is_contiguous() and cls.is_contiguous() and pos.is_contiguous()) or tuple(pos.shape) != (1 + n_p, c) or cls.numel() != c:
        raise ValueError("vit_tokens_f32: patches contiguous [b * np, C], cls [C], pos contiguous [1 + np, C]")
    out = torch.empty((b * (1 + n_p + tail_rows), c), dtype=F32, device=patches.device)
    check(_lib.lib().avsd_vit_tokens_f32(_p(patches), _p(cls), _p(pos), _p(out), b, n_p, c, tail_rows, _stream()), "avsd_vit_tokens_f32")
    return out


def cosine_rows_f32(x: torch.Tensor, y: torch.Tensor, rep: int = 1) -> torch.Tensor:
    """x [m, C], y [m / rep, C] f32 -> [m]: the cosine of row i of x and row i // rep of y, norms clamped at 1e-12 as F.normalize"""
    _req(x, F32, "x")
    _req(y, F32, "y")
    if x.dim() != 2 or y.dim() != 2 or not x.is_contiguous() or not y.is_contiguous() or x.shape[1] != y.shape[1] or rep < 1 \
            or y.shape[0] * rep != x.shape[0]:
        raise ValueError(f"cosine_rows_f32: x contiguous [m, C] and y contiguous [m / rep, C], got {tuple(x.shape)}, {tuple(y.shape)}, rep {rep}")
    out = torch.empty((x.shape[0],), dtype=F32, device=x.device)
    check(_lib.lib().avsd_cosine_rows_f32(_p(x), _p(y), _p(out), x.shape[0], x.shape[1], rep, _stream()), "avsd_cosine_rows_f32")
    return out


def normalize_rows_f32(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [m, C] contiguous f32 -> rows divided by max(their L2 norm, 1e-12), as F.normalize; `out` may be x"""
    _req(x, F32, "x")
    out = torch.empty_like(x) if out is None else out
    _req(out, F32, "out")
    if x.dim() != 2 or not x.is_contiguous() or not out.is_contiguous() or tuple(out.shape) != tuple(x.shape):
        raise ValueError("normalize_rows_f32: x and out must be contiguous [m, C]")
    check(_lib.lib().avsd_normalize_rows_f32(_p(x), _p(out), x.shape[0], x.shape[1], _stream()), "avsd_normalize_rows_f32")
    return out
