"""Cases of the codec record tests (test_gpu_codec_records.py): frames whose RIRB1 records are DESIGNED - the mode, the eight block
widths and the base of every record are chosen first and the pixels made to fit - so that the expected header is known without running
any codec, and so that the records the other codec tests never make do occur: MODE_LEFT key records, widths that differ inside a record,
the step between the narrow tier (all widths <= 4) and the wide one, and the tie of the key-mode rule.  header_fields and census read
headers back as the format text says (oracle/rir_oracle.c, the comment above TILE_PX), independently of the oracle's code; the CPU suite
asserts with them that the cases reach what they are for (test_codec_cases_cpu.py).  numpy only: no GPU, no library call, no test
function."""
import functools

import numpy as np

TILE_PX = 512  # RIRB1_TILE_PX: lane l of a tile holds pixels 8l .. 8l + 7, block j the 64 pixels 8l + j
MODE_RAW, MODE_TEMPORAL, MODE_LEFT = 0, 1, 2
NARROW_MAX = 4  # a record whose widths are all <= 4 is written by the narrow tier

PATTERNS = ([[(k + 5 * j) % 17 for j in range(8)] for k in range(17)]  # every (block, width) pair, mixed within each record
            + [[(k + 2 * j) % 5 for j in range(8)] for k in range(5)]  # every pair with width <= 4, all widths <= 4: the narrow tier, mixed
            + [[5 if j == s else (s + 2 * j) % 5 for j in range(8)] for s in range(8)]  # one step over the tier edge, at each block
            + [[k] * 8 for k in range(17)])  # uniform
NPATTERNS = len(PATTERNS)  # 47
LEFT_WIDEST = [16] * 7 + [15]  # stands for [16] * 8 in a LEFT key record: with eight widths of 16 the tie goes to RAW

SCENE_H, SCENE_W = 94, 256  # 47 whole tiles
SCENE_FRAMES = 48


def residuals(rng, widths):
    """512 residuals, pixel 8l + j in block j: block j's OR has bit length widths[j] exactly and the tile's minimum is 0"""
    r = np.zeros((64, 8), np.int64)
    for j, w in enumerate(widths):
        if w:
            r[:, j] = rng.integers(0, 1 << w, 64)
            r[rng.integers(0, 64), j] |= 1 << (w - 1)
    if min(widths) > 0:  # (a block of width 0 is all zeros already)
        l, j = rng.integers(0, 64), rng.integers(0, 8)
        r[l, j] = 0
        if np.bitwise_or.reduce(r[:, j]) >> (widths[j] - 1) == 0:  # that element alone held the top bit
            r[(l + 1) % 64, j] |= 1 << (widths[j] - 1)
    return r.reshape(-1)


def offset(rng, widths, signed):
    """c such that c + r does not cross the wrap of the compare (signed int16 or unsigned): the low end, the high end or a random value"""
    top = (1 << max(widths)) - 1
    lo, hi = (-32768, 32767 - top) if signed else (0, 65535 - top)
    return int(rng.choice([lo, hi, rng.integers(lo, hi + 1)]))


def _key_widths(pattern, key):
    return LEFT_WIDEST if key == "left" and min(pattern) == 16 else list(pattern)


def _key_tile(rng, widths, key):
    """(pixels before the reduction mod 2^16, c) of a designed key record: c + r itself (RAW), or its running sum (LEFT: d = c + r)"""
    c = offset(rng, widths, key == "left")
    d = c + residuals(rng, widths)
    return (np.cumsum(d) if key == "left" else d), c


@functools.lru_cache(maxsize=None)
def _record_scene(seed, key, nframes):
    rng = np.random.default_rng(seed)
    fr = np.zeros((nframes, NPATTERNS, TILE_PX), np.int64)
    mode = np.full((NPATTERNS, nframes), MODE_TEMPORAL)
    mode[:, 0] = MODE_LEFT if key == "left" else MODE_RAW
    widths = np.zeros((NPATTERNS, nframes, 8), int)
    base = np.zeros((NPATTERNS, nframes), np.int64)
    for t in range(NPATTERNS):
        widths[t, 0] = _key_widths(PATTERNS[t], key)
        fr[0, t], base[t, 0] = _key_tile(rng, list(widths[t, 0]), key)
        for f in range(1, nframes):
            w = PATTERNS[(t + f) % NPATTERNS]
            c = offset(rng, w, True)
            fr[f, t] = fr[f - 1, t] + c + residuals(rng, w)
            widths[t, f], base[t, f] = w, c
    out = (fr % 65536).astype(np.uint16).reshape(nframes, SCENE_H, SCENE_W)
    for a in (out, mode, widths, base):
        a.setflags(write=False)
    return out, mode, widths, base % 65536


@functools.lru_cache(maxsize=None)
def _key_scene(seed, key, n):
    rng = np.random.default_rng(seed)
    fr = np.zeros((n, NPATTERNS, TILE_PX), np.int64)
    widths = np.zeros((n, NPATTERNS, 8), int)
    base = np.zeros((n, NPATTERNS), np.int64)
    for i in range(n):
        for t in range(NPATTERNS):
            widths[i, t] = _key_widths(PATTERNS[(t + i) % NPATTERNS], key)
            fr[i, t], base[i, t] = _key_tile(rng, list(widths[i, t]), key)
    out = (fr % 65536).astype(np.uint16).reshape(n, SCENE_H, SCENE_W)
    mode = np.full((n, NPATTERNS), MODE_LEFT if key == "left" else MODE_RAW)
    for a in (out, mode, widths, base):
        a.setflags(write=False)
    return out, mode, widths, base % 65536


def record_scene(seed, key, nframes=SCENE_FRAMES):
    """uint16 [nframes][94][256] (read-only), 47 whole tiles, to be encoded as ONE chunk: tile t's key record is PATTERNS[t] in mode `key`
    ("raw" or "left"), frame f > 0 is the frame before plus c + r of PATTERNS[(t + f) % 47]: every pattern stands at every frame position
    of the chunk in some tile, and so in every wave and walking direction of an encoder that splits a chunk's frames among waves"""
    return _record_scene(seed, key, nframes)[0]


def key_scene(seed, key, n=3):
    """uint16 [n][94][256] (read-only) of independent designed key frames for GOP 1: tile t of frame i is PATTERNS[(t + i) % 47]"""
    return _key_scene(seed, key, n)[0]


def design(scene, seed, key, n=None):
    """the designed (mode, widths, base = c mod 2^16) of every record of record_scene (scene "record": arrays [tile][frame], for the
    scene encoded as one chunk) or key_scene (scene "key": arrays [frame][tile], for GOP 1)"""
    if scene == "record":
        return _record_scene(seed, key, SCENE_FRAMES if n is None else n)[1:]
    if scene == "key":
        return _key_scene(seed, key, 3 if n is None else n)[1:]
    raise ValueError(scene)


# ---- the key-mode rule: LEFT only when strictly smaller --------------------------------------------------------------------------------
TIE_TILE = np.tile([2, 3, 2, 3, 1, 2, 0, 1], 64)  # RAW and LEFT both cost 12 words: RAW
LEFT_BY_ONE_TILE = np.tile([18, 17, 21, 31, 31, 22, 9, 5], 64)  # RAW costs 31 words, LEFT 30: LEFT
TIE_WORDS = {"tie": (12, 12), "left_by_one": (31, 30)}  # (RAW, LEFT) payload words, counted by hand


def mode_totals(tile):
    """(RAW words, LEFT words) of a key tile of 512 pixels: a plain count from the format text"""
    p = np.asarray(tile, np.int64) % 65536
    d = (p - np.concatenate([[0], p[:-1]])) % 65536
    d = np.where(d >= 32768, d - 65536, d)

    def words(r):
        return sum(int(np.bitwise_or.reduce(r.reshape(64, 8)[:, j])).bit_length() for j in range(8))

    return words(p - p.min()), words(d - d.min())


def tie_frames():
    """uint16 [3][2][1024], 4 tiles: the two hand tiles side by side in both orders in frame 0 and, swapped, in frame 1 (both are key
    frames at GOP 1); frame 2 is frame 1 plus designed residuals"""
    a, b = TIE_TILE, LEFT_BY_ONE_TILE
    f0, f1 = np.concatenate([a, b, b, a]), np.concatenate([b, a, a, b])
    rng = np.random.default_rng(17)
    f2 = f1 + np.concatenate([offset(rng, PATTERNS[k], True) + residuals(rng, PATTERNS[k]) for k in (3, 18, 24, 40)])
    return (np.stack([f0, f1, f2]) % 65536).astype(np.uint16).reshape(3, 2, 2 * TILE_PX)


# ---- frames that are no whole tiles, frame pointers off the 16-byte grid ---------------------------------------------------------------
RAGGED_CUT = (3, 7937)  # 46 * 512 + 259 pixels: no multiple of 8
RAGGED_RAMP = (3, 2817)  # 16 * 512 + 259


def ramp_frames():
    """uint16 [3][3][2817]: pixel p of frame 0 is 30000 + 100 (p % 512), then two noisy frames.  Every key record, the zero-padded last
    tile's included, is LEFT (test_codec_cases_cpu.py asserts it)."""
    h, w = RAGGED_RAMP
    npx = h * w
    rng = np.random.default_rng(3)
    fr = np.zeros((3, npx), np.int64)
    fr[0] = 30000 + 100 * (np.arange(npx) % TILE_PX)
    fr[1] = fr[0] + rng.integers(-3, 4, npx)
    fr[2] = fr[1] + rng.integers(-300, 400, npx)
    return (fr % 65536).astype(np.uint16).reshape(3, h, w)


def ragged_scene(seed=11):
    """[(name, frames, elements the frame pointer is off the 16-byte grid)]: the first 46 * 512 + 259 pixels of the LEFT record scene;
    the ramp; the whole-tile record scenes behind a pointer 1 and 3 elements off"""
    h, w = RAGGED_CUT
    left, raw = record_scene(seed, "left"), record_scene(seed, "raw")
    cut = np.ascontiguousarray(left.reshape(left.shape[0], -1)[:, :h * w]).reshape(-1, h, w)
    return [("left_cut", cut, 0), ("ramp", ramp_frames(), 0), ("raw_off1", raw, 1), ("raw_off3", raw, 3), ("left_off1", left, 1), ("left_off3", left, 3)]


# ---- headers, read back from the format text ---------------------------------------------------------------------------------------------
def header_fields(hdr):
    """(mode, widths[..., 8], base) of uint64 headers of any shape.  Four 16-bit fields, field q at bits [16q, 16q + 16): bits 0-4 w_q,
    bits 5-9 w_{4+q}, bits 10-13 nibble q of the base, bits 14-15 the mode (field 0 only)."""
    h = np.asarray(hdr).astype(np.uint64)
    field = [((h >> np.uint64(16 * q)) & np.uint64(0xFFFF)).astype(np.int64) for q in range(4)]
    widths = np.stack([f & 31 for f in field] + [(f >> 5) & 31 for f in field], axis=-1)
    base = sum(((f >> 10) & 15) << (4 * q) for q, f in enumerate(field))
    assert not any(((f >> 14) & 3).any() for f in field[1:]), "bits 14-15 of fields 1..3 are never set"
    return (field[0] >> 14) & 3, widths, base


def tier_class(widths):
    """the class of one record's widths: ("uniform", w); "narrow_mixed" (all <= 4, not all equal); "tier_edge" (exactly one block at 5,
    the rest <= 4); "wide_mixed" (every other record)"""
    w = [int(x) for x in widths]
    if len(set(w)) == 1:
        return ("uniform", w[0])
    if max(w) <= NARROW_MAX:
        return "narrow_mixed"
    if sorted(w)[-1] == NARROW_MAX + 1 and sorted(w)[-2] <= NARROW_MAX:
        return "tier_edge"
    return "wide_mixed"


def census_of_headers(hdr):
    """(cells, classes) of uint64 headers: the set of (mode, block, width) and the set of (mode, tier_class) that occur"""
    mode, widths, _ = header_fields(hdr)
    mode, widths = mode.reshape(-1), widths.reshape(-1, 8)
    cells, classes = set(), set()
    for m, w in {(int(m), tuple(int(x) for x in w)) for m, w in zip(mode, widths)}:
        cells |= {(m, j, w[j]) for j in range(8)}
        classes.add((m, tier_class(w)))
    return cells, classes


def census(frames, gop, oracle):
    """per chunk of `frames` at `gop`, (cells, classes) of the records the oracle makes of it"""
    return [census_of_headers(oracle.codec_encode_chunk(np.ascontiguousarray(frames[f0:f0 + gop]))[0]) for f0 in range(0, frames.shape[0], gop)]


ALL_CELLS = {(m, j, w) for m in (MODE_RAW, MODE_TEMPORAL, MODE_LEFT) for j in range(8) for w in range(17)}  # 408
