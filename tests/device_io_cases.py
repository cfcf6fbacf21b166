"""Cases of the device I/O tests (IRMovie.to_tensor / rir_load_images_device, IRSaver.add_images / rir_add_images_device) over the full
16-bit range: the frames, MIN_T as numpy defines it, and plain restatements of two pieces of the library's arithmetic - which of a lane's
eight pixels get MIN_T in rirb1_decode_select (codec_kernels.hip) and which chunk jobs and batches load_images_device (video_io_abi.cpp)
makes of a selection - so that the CPU suite can assert that the case tables reach the paths they are there for
(test_device_io_cases_cpu.py).  numpy only: no GPU, no library call, no test function."""
import numpy as np

from librir_amd.synthetic import s1_noisy_background

TILE_PX = 512  # RIRB1_TILE_PX: pixels of a tile, 8 per lane of a wave
# load_images_device's batch limits (kDioBatchChunks, kDioBatchBytes, kDioScratchBytes: the CPU test reads them from the source)
BATCH_CHUNKS = 8
BATCH_BYTES = 64 << 20
SCRATCH_BYTES = 256 << 20

KINDS = ("uniform", "extremes", "high")
SPECIALS = (0, 32767, 32768, 65535)


def frames(kind, n, h, w, seed):
    """uint16 [n][h][w] of `kind`"""
    rng = np.random.default_rng(seed)
    npx = h * w
    if kind == "uniform":
        return rng.integers(0, 65536, (n, h, w)).astype(np.uint16)
    if kind == "extremes":  # a 0 / 65 535 checkerboard that flips every frame: every residual is +-65 535
        yy, xx = np.mgrid[0:h, 0:w]
        board = (yy + xx) & 1
        return np.stack([np.where(board ^ (i & 1), 65535, 0) for i in range(n)]).astype(np.uint16)
    if kind == "high":  # bit 15 set everywhere, the four special values at the frame's and at every tile's first and last pixel
        out = (32768 + rng.integers(0, 40, (n, npx))).astype(np.uint16)
        edges = sorted({0, npx - 1} | {p for t in range(0, npx, TILE_PX) for p in (t, min(t + TILE_PX, npx) - 1)})
        for i in range(n):
            for j, p in enumerate(edges):
                out[i, p] = SPECIALS[(i + j) % 4]
        return out.reshape(n, h, w)
    if kind == "s1_high":  # compressible, near the top of the range (<= 65 024 + n)
        return (s1_noisy_background(n, h, w, seed).astype(np.int64) + 64000).astype(np.uint16)
    raise ValueError(kind)


def with_ends(arr):
    """`arr` with two pixels of every 16 at 65 535 and two at 0 .. 4, the values that wrap when MIN_T is as small as 1 or -5 - one of each
    at an odd and one at an even position: the high and the low half of a packed pair (a carry out of the low half is the one that shows)"""
    n, h, w = arr.shape
    out = arr.copy().reshape(n, -1)
    small = (np.arange(n, dtype=np.uint16) % 5)[:, None]
    out[:, 3::16] = 65535
    out[:, 6::16] = 65535
    out[:, 11::16] = small
    out[:, 12::16] = small
    return out.reshape(n, h, w)


def min_t_rows(h, min_t_height):
    """rows that get MIN_T: MIN_T_HEIGHT, h - 3 when it is absent (0), never more than the frame has"""
    return h - 3 if min_t_height == 0 else min(min_t_height, h)


def min_t_expected(arr, min_t, min_t_height):
    """what a reader gives for stored frames `arr`: MIN_T added to the first rows, as an unsigned short += does (it wraps)"""
    rows = min_t_rows(arr.shape[1], min_t_height)
    out = arr.copy()
    out[:, :rows] = (arr[:, :rows].astype(np.int64) + min_t).astype(np.uint16)
    return out


def lane_classes(h, w, rows):
    """(nmin values met in whole tiles, nmin values met in the cut last tile, whole tiles): lane `lane` of tile `tile` holds the pixels
    p0 .. p0 + 7, p0 = tile * 512 + lane * 8, and adds MIN_T to the first nmin = clamp(w * rows - p0, 0, 8) of them.  Whole tiles (the
    FAST instantiation) exist only in frames whose pixel count is a multiple of 8; every other tile counts as cut."""
    npx, min_px = h * w, w * rows
    whole = npx // TILE_PX if npx % 8 == 0 else 0
    in_whole, in_cut = set(), set()
    for p0 in range(0, npx, 8):
        (in_whole if p0 // TILE_PX < whole else in_cut).add(max(0, min(8, min_px - p0)))
    return in_whole, in_cut, whole


def read_plan(n, gop, first, count, step):
    """The batches load_images_device cuts images first + k * step (k < count) of an n-image recording into, each a list of chunk jobs
    (chunk, first selected frame within the chunk, selected frames, first output slot); chunks without a selected frame have no job; a
    batch holds at most BATCH_CHUNKS jobs.  (The byte and scratch limits are ignored: test_device_io_cases_cpu.py shows why it may.)"""
    jobs = []
    for c in range((n + gop - 1) // gop):
        cf, cn = c * gop, min(gop, n - c * gop)
        k_lo, k_hi = max(0, -((first - cf) // step)), min(count, -((first - cf - cn) // step))
        if cf + cn <= first or k_hi <= k_lo:
            continue
        jobs.append((c, first + k_lo * step - cf, k_hi - k_lo, k_lo))
    assert sum(j[2] for j in jobs) == count
    return [jobs[i:i + BATCH_CHUNKS] for i in range(0, len(jobs), BATCH_CHUNKS)]


def plan_of(n, gop, sel):
    """read_plan of a slice or an int as IRMovie.to_tensor takes them"""
    r = range(n)[sel] if isinstance(sel, slice) else range(sel % n, sel % n + 1)
    return read_plan(n, gop, r.start, len(r), r.step) if len(r) else []


def selections(n, gop):
    """the selections of the lossless reads: steps around the GOP, single frames at the chunks' ends, empty ones"""
    g = min(gop, n)
    sels = [slice(None, None, s) for s in sorted({1, gop - 1, gop, gop + 1, 2 * gop + 1}) if s >= 1]
    sels += [slice(g - 1, None, gop), slice(1, None, gop + 1)]  # the last frame of every chunk alone; a drifting phase
    sels += sorted({0, g - 1, min(g, n - 1), n - 1})  # frame 0, chunk 0's last, chunk 1's first, the (short) last chunk's last
    sels += [slice(5, 5), slice(8, 2)]
    return sels


# ---- the case tables --------------------------------------------------------------------------------------------------------------

DEFAULT_GOP = 50
LOSSLESS_SHAPES = [(1, 1), (1, 8), (16, 32), (32, 44), (9, 13), (67, 83), (3, 1025)]
# (gop, n): a short last chunk; no short chunk; and on two shapes GOP 1 and the default GOP (None: larger than the recording)
LOSSLESS_RECORDINGS = [(3, 11), (4, 12)]
LOSSLESS_EXTRA_SHAPES = [(32, 44), (9, 13)]
LOSSLESS_EXTRA_RECORDINGS = [(1, 9), (None, 7)]
RAW_SHAPE, RAW_N = (40, 72), 17  # the PCR and ZFile recordings

# (h, w, MIN_T_HEIGHT): 32x44 = 2 whole tiles + a cut one, with the boundary inside a lane of tile 0, of tile 1 and of the cut tile;
# 9x13: no whole tile (117 pixels); 16x32: exactly one whole tile, boundary on a lane's edge
MIN_T_GEOMETRIES = [(32, 44, 1), (32, 44, 13), (32, 44, 29), (9, 13, 4), (16, 32, 5)]
MIN_T_VALUES = [1, 40000, 65535, -5]
MIN_T_RECORDING = (3, 11)  # (gop, n)
MIN_T_SELECTIONS = [slice(None), slice(None, None, 2), slice(2, None, 3), slice(4, 9), 10]
# MIN_T in a second and a third batch
MIN_T_LONG = dict(h=32, w=44, n=37, gop=2, min_t=40000, rows=13, selections=[slice(None), slice(None, None, 3)])

OUT_SHAPES = [(32, 44), (16, 32)]
OUT_RECORDING = (3, 11)
OUT_STEPS = [1, 2, 3, 4]
OUT_OFFSETS = {"uint16": (0, 1, 4, 8), "float32": (0, 1, 2, 4)}  # elements past the allocation's (16-byte aligned) start

# filtered reads: 3 batches; skipped chunks; a start inside the recording and beyond the first batch; one frame per job
FILTERED = dict(h=40, w=72, n=37, gop=2, selections=[slice(None), slice(1, None, 3), slice(17, 36), slice(0, None, 5)])

# the two large reads: the byte cut (incompressible chunks) and the scratch cut (float32 + motion: two scratch frames per image)
LARGE = dict(h=512, w=640, n=210, gop=50, base=10)

WRITE_SHAPES = [(32, 44), (9, 13), (16, 32), (67, 83)]
WRITE_RECORDING = (3, 11)
WRITE_PIECES = [(0, 1), (1, 3), (3, 3), (3, 6), (6, 11)]
WRITE_OFFSETS = [1, 4]


def small_recordings():
    """(n, h, w, gop) of every recording of the GPU tests but the two of LARGE"""
    out = [(n, h, w, gop or DEFAULT_GOP) for h, w in LOSSLESS_SHAPES for gop, n in LOSSLESS_RECORDINGS]
    out += [(n, h, w, gop or DEFAULT_GOP) for h, w in LOSSLESS_EXTRA_SHAPES for gop, n in LOSSLESS_EXTRA_RECORDINGS]
    out += [(MIN_T_RECORDING[1], h, w, MIN_T_RECORDING[0]) for h, w, _ in MIN_T_GEOMETRIES]
    out += [(d["n"], d["h"], d["w"], d["gop"]) for d in (MIN_T_LONG, FILTERED)]
    out += [(OUT_RECORDING[1], h, w, OUT_RECORDING[0]) for h, w in OUT_SHAPES]
    out += [(WRITE_RECORDING[1], h, w, WRITE_RECORDING[0]) for h, w in WRITE_SHAPES]
    return out


def batch_bytes_bound(h, w, gop, chunks, frames_in):
    """an upper bound of the page-locked bytes of a batch of `chunks` chunks that hold `frames_in` images: per chunk the select entry, the
    chunk offset, the record headers and the tile offsets, plus a payload no record of which is longer than RIRB1_REC_MAX_WORDS = 128
    words (16-bit-wide records: the tile's raw size)"""
    ntiles = (h * w + TILE_PX - 1) // TILE_PX
    return chunks * (ntiles * gop * 8 + (ntiles + 1) * 4 + 32) + frames_in * ntiles * 128 * 8 + 8


def large_frames(kind, seed):
    """LARGE's frames: `base` frames of `kind` tiled along time, pixel (0, 0) of frame i set to i - no two frames are equal"""
    d = LARGE
    arr = np.tile(frames(kind, d["base"], d["h"], d["w"], seed), (d["n"] // d["base"], 1, 1))
    arr[:, 0, 0] = np.arange(d["n"])
    return arr
