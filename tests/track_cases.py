"""Helper of the component-tracking tests (not a test module): the numpy oracle of rir_track_components_device, a brute-force restatement
of its definition for tiny stacks, and the generators of the scenes the tests use."""
import numpy as np

TABLES = ("first_frame", "last_frame", "first_label", "components")
RANDOM_SHAPES = [(1, 1, 1), (2, 3, 5), (3, 4, 7), (70, 9, 67), (5, 40, 300), (130, 6, 11)]  # (n, h, w), at densities 0.45-0.55


def limits(n, nlabels, counts):
    """per frame: label k names a component when 1 <= k < limit"""
    if counts is None:
        return np.full(n, nlabels, np.int64)
    return np.maximum(1, np.minimum(nlabels, np.asarray(counts, np.int64)))


def default_table_entries(n, nlabels):
    return min(n * (nlabels - 1) + 1, 65536)


def track_oracle(labels, counts=None, nlabels=None, table_entries=None):
    """the contract with a union-find over (t, k) pairs taken from set(zip(a, b)) per frame pair, roots = lowest node, tracks numbered by
    lowest node.  -> dict: track_of [n][K], info [2], the four tables [T], tracks [n][h][w] (all int32) and volume [ntracks] (int64)"""
    labels = np.asarray(labels)
    n, h, w = labels.shape
    K = int(nlabels)
    T = default_table_entries(n, K) if table_entries is None else int(table_entries)
    lim = limits(n, K, counts)
    parent = list(range(n * K))

    def find(i):
        r = i
        while parent[r] != r:
            r = parent[r]
        while parent[i] != r:
            parent[i], i = r, parent[i]
        return r

    flat = labels.reshape(n, -1).astype(np.int64)
    for t in range(n - 1):
        a, b = flat[t], flat[t + 1]
        ok = (a >= 1) & (a < lim[t]) & (b >= 1) & (b < lim[t + 1])
        for x, y in set(zip(a[ok].tolist(), b[ok].tolist())):
            ra, rb = find(t * K + x), find((t + 1) * K + y)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    k = np.arange(K)
    exists = (k[None, :] >= 1) & (k[None, :] < lim[:, None])
    nodes = np.flatnonzero(exists.reshape(-1))
    root = np.array([find(int(i)) for i in nodes], np.int64)
    roots = np.unique(root)  # sorted: the order of the lowest nodes
    ntracks = len(roots) + 1
    track_of = np.zeros(n * K, np.int32)
    number = np.searchsorted(roots, root) + 1
    track_of[nodes] = number
    tab = {"first_frame": np.zeros(T, np.int32), "last_frame": np.zeros(T, np.int32), "first_label": np.zeros(T, np.int32),
           "components": np.zeros(T, np.int32)}
    tab["first_frame"][0] = tab["last_frame"][0] = -1
    keep = number < T
    tr, fr = number[keep], nodes[keep] // K
    m = min(ntracks, T)
    tab["first_frame"][1:m] = (roots // K)[:m - 1]
    tab["first_label"][1:m] = (roots % K)[:m - 1]
    np.maximum.at(tab["last_frame"], tr, fr.astype(np.int32))
    np.add.at(tab["components"], tr, 1)
    track_of = track_of.reshape(n, K)
    valid = (flat >= 1) & (flat < lim[:, None])
    tracks = np.where(valid, np.take_along_axis(track_of, np.where(valid, flat, 0), axis=1), 0).astype(np.int32).reshape(n, h, w)
    dropped = 0 if counts is None else int((np.asarray(counts) > K).sum())
    out = {"track_of": track_of, "info": np.array([ntracks, dropped], np.int32), "tracks": tracks,
           "volume": np.bincount(tracks.reshape(-1), minlength=ntracks).astype(np.int64)}
    out.update(tab)
    return out


def brute_force(labels, counts, nlabels, table_entries):
    """the definition word for word: components that exist, links found pixel by pixel, tracks by flooding the link graph from the lowest
    unvisited node, tables by a loop over the members of each track"""
    n, h, w = labels.shape
    K, T = nlabels, table_entries
    lim = [K if counts is None else max(1, min(K, int(counts[t]))) for t in range(n)]
    exists = [[1 <= k < lim[t] for k in range(K)] for t in range(n)]
    linked = set()
    for t in range(n - 1):
        for y in range(h):
            for x in range(w):
                a, b = int(labels[t, y, x]), int(labels[t + 1, y, x])
                if 0 <= a < K and 0 <= b < K and exists[t][a] and exists[t + 1][b]:
                    linked.add((t * K + a, (t + 1) * K + b))
    near = {}
    for a, b in linked:
        near.setdefault(a, set()).add(b)
        near.setdefault(b, set()).add(a)
    track_of = np.zeros((n, K), np.int32)
    members = [None]
    for node in range(n * K):
        if not exists[node // K][node % K] or track_of[node // K, node % K]:
            continue
        todo, mine = [node], {node}
        while todo:
            for o in near.get(todo.pop(), ()):
                if o not in mine:
                    mine.add(o)
                    todo.append(o)
        members.append(sorted(mine))
        for o in mine:
            track_of[o // K, o % K] = len(members) - 1
    tab = {k: np.zeros(T, np.int32) for k in TABLES}
    tab["first_frame"][0] = tab["last_frame"][0] = -1
    for tr in range(1, min(len(members), T)):
        mine = members[tr]
        tab["first_frame"][tr], tab["last_frame"][tr] = mine[0] // K, max(o // K for o in mine)
        tab["first_label"][tr], tab["components"][tr] = mine[0] % K, len(mine)
    tracks = np.zeros((n, h, w), np.int32)
    for t in range(n):
        for y in range(h):
            for x in range(w):
                a = int(labels[t, y, x])
                if 0 <= a < K and exists[t][a]:
                    tracks[t, y, x] = track_of[t, a]
    dropped = 0 if counts is None else sum(int(c) > K for c in counts)
    out = {"track_of": track_of, "info": np.array([len(members), dropped], np.int32), "tracks": tracks}
    out.update(tab)
    return out


def random_mask(seed, n, h, w):
    rng = np.random.default_rng(seed)
    return rng.random((n, h, w)) < rng.uniform(0.45, 0.55)


def random_labels(seed, n, h, w, nlabels, with_counts=True):
    """label maps no labelling produced: values from -2 to nlabels + 2, counts on both sides of nlabels"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(-2, nlabels + 3, (n, h, w)).astype(np.int32)
    labels.reshape(-1)[::13] = np.iinfo(np.int32).min
    labels.reshape(-1)[5::17] = np.iinfo(np.int32).max
    counts = rng.integers(0, nlabels + 4, n).astype(np.int32) if with_counts else None
    return labels, counts


def late_merge(m, n, joined_first):
    """m separate one-pixel-wide columns through n frames, and a full row that joins them all in the last frame (or in the first)"""
    mask = np.zeros((n, 4, 2 * m), bool)
    mask[:, 1:, ::2] = True
    mask[0 if joined_first else n - 1, 1, :] = True
    return mask


def staircase(n, h, w):
    """a 2-pixel blob that moves one pixel a frame along the rows from row 2 on, turning into the next row at a row's end (rows run left
    to right and right to left in turn, so the blob stays one component); up to three single pixels come and go in row 0, before the blob
    in raster order, so the blob's label changes from frame to frame"""
    assert n + 1 <= (h - 2) * w
    path = [(y, x if (y - 2) % 2 == 0 else w - 1 - x) for y in range(2, h) for x in range(w)]
    mask = np.zeros((n, h, w), bool)
    for t in range(n):
        mask[t][path[t]] = mask[t][path[t + 1]] = True
        mask[t, 0, 0:2 * (t % 4):2] = True
    return mask


def comb(h, w, teeth_first):
    """every second column its own component in one frame, one component over everything in the other"""
    mask = np.ones((2, h, w), bool)
    mask[0 if teeth_first else 1, :, 1::2] = False
    return mask


def checkerboards(n, h, w):
    """complementary checkerboards in alternating frames: every pixel of a frame its own component, no pixel set in two adjacent frames"""
    t, y, x = np.mgrid[0:n, 0:h, 0:w]
    return (t + y + x) % 2 == 0
