"""TEST INFRASTRUCTURE for the device neighbour search (include/gpak_dev_local_search.h, include/gpak_local_search.h),
written from the headers alone, in NumPy:

* grid(T, h): the samples binned into a uniform cell grid of a CHOSEN cell size by the rule the kernel may assume -- cell
  a_j = min(max(floor((t_j - lo_j) / h), 0), n_j - 1), a stable counting sort so that the indices ascend inside a cell,
  start the running count over the cells (cell index (a0 n1 + a1) n2 + a2), scale = max |lo_j|, |hi_j|;
* check_grid: those invariants, asserted;
* dist2_lists: dist2 of every listed sample in the stated arithmetic (every difference, product and sum rounded on its
  own, j ascending), 0.0 in the unused slots;
* kernel_cases: the grids the kernel is run on alone (tests/local_search_worker.py), shared with the CPU test that asserts
  they have the properties they were chosen for.
The lists themselves come from local_ref.brute_neighbours (a full sort)."""
import numpy as np


def transform(X, G):
    """t_j = ((x_0 G_0j + x_1 G_1j) + x_2 G_2j) [+ x_3 G_3j]; None: the identity"""
    X = np.asarray(X, dtype=np.float64)
    if G is None:
        return X.copy()
    G = np.asarray(G, dtype=np.float64)
    cols = []
    for j in range(X.shape[1]):
        t = X[:, 0] * G[0, j]
        for r in range(1, X.shape[1]):
            t = t + X[:, r] * G[r, j]
        cols.append(t)
    return np.column_stack(cols)


def grid(T, h):
    """T: n x d transformed samples; returns a dict pts (n x d, cell order), ids (int32), start (int32, cells + 1), lo (3),
    n (3 ints), h, scale"""
    T = np.asarray(T, dtype=np.float64)
    lo, hi = T[:, :3].min(axis=0), T[:, :3].max(axis=0)
    n = [int(np.floor((hi[j] - lo[j]) / h)) + 1 for j in range(3)]
    a = [np.clip(np.floor((T[:, j] - lo[j]) / h), 0, n[j] - 1).astype(np.int64) for j in range(3)]
    cell = (a[0] * n[1] + a[1]) * n[2] + a[2]
    order = np.argsort(cell, kind="stable")
    start = np.zeros(n[0] * n[1] * n[2] + 1, dtype=np.int64)
    np.add.at(start, cell + 1, 1)
    start = np.cumsum(start)
    return {"pts": np.ascontiguousarray(T[order]), "ids": order.astype(np.int32), "start": start.astype(np.int32), "lo": lo, "n": n,
            "h": float(h), "scale": float(max(np.abs(lo).max(), np.abs(hi).max())), "cell": cell}


def check_grid(g, T):
    """what gpak_dev_local_search may assume of a grid"""
    n, lo, h, start, ids = g["n"], g["lo"], g["h"], g["start"].astype(np.int64), g["ids"]
    nc = n[0] * n[1] * n[2]
    assert start.shape == (nc + 1,) and start[0] == 0 and start[-1] == len(T) and np.all(np.diff(start) >= 0)
    assert sorted(ids.tolist()) == list(range(len(T))) and np.array_equal(g["pts"], T[ids])
    for c in np.flatnonzero(np.diff(start)):
        inside = ids[start[c]:start[c + 1]]
        assert np.all(np.diff(inside) > 0)                                   # ascending inside a cell
        a = (c // (n[1] * n[2]), (c // n[2]) % n[1], c % n[2])
        for j in range(3):
            want = np.clip(np.floor((T[inside, j] - lo[j]) / h), 0, n[j] - 1)
            assert np.all(want == a[j])
    assert g["scale"] >= np.abs(T[:, :3]).max()


def host_cell_size(T):
    """about the cell size gpak_local_neighbours chooses: four samples per cell over the dimensions with an extent"""
    ext = T[:, :3].max(axis=0) - T[:, :3].min(axis=0)
    live = ext[ext > 0.0]
    return float((np.prod(live) / max(1.0, len(T) / 4.0)) ** (1.0 / len(live))) if len(live) else 1.0


def dist2_to(T, tc):
    e = T[:, 0] - tc[0]
    d2 = e * e
    for j in range(1, T.shape[1]):
        e = T[:, j] - tc[j]
        d2 = d2 + e * e
    return d2


def dist2_lists(Ts, Tc, nbr):
    """M x k: dist2 of the samples nbr names, 0.0 where it holds -1"""
    out = np.zeros(nbr.shape)
    for b in range(nbr.shape[0]):
        live = nbr[b] >= 0
        out[b, live] = dist2_to(Ts, Tc[b])[nbr[b, live]]
    return out


def visited_floor(Ts, Tc, nbr, k, radius):
    """samples the search cannot have skipped: per centre those at most as far as its list reaches -- the worst listed dist2
    of a full list, else everything (inside the radius when there is one)"""
    total = 0
    for b in range(len(Tc)):
        d2 = dist2_to(Ts, Tc[b])
        used = int((nbr[b] >= 0).sum())
        reach = d2[nbr[b, k - 1]] if used == k else np.inf
        if radius > 0.0:
            reach = min(reach, radius * radius)
        total += int((d2 <= reach).sum())
    return total


KERNEL_INPUTS = ("random", "d4")
KERNEL_GRIDS = ("one-cell", "tenth", "own")
KERNEL_K = (17, 128)


def kernel_case(inputs, which):
    """(Ts, Tc, G, grid): the transformed samples and centres of tests/test_local.py's `inputs` -- the centres followed by one
    outside the samples' box on each side of each axis and one 1e6 away -- and the grid `which`:
    one-cell (every span longer than 64), tenth (a tenth of the host's cell size: mostly empty cells, many rings), own"""
    from test_local import search_inputs
    Xs, Xc, G = search_inputs(inputs)
    Ts, Tc = transform(Xs, G), transform(Xc, G)
    lo, hi = Ts.min(axis=0), Ts.max(axis=0)
    mid, ext = 0.5 * (lo + hi), (hi - lo)[:3].max()
    extra = []
    for j in range(3):
        for side in (-1.0, 1.0):
            p = mid.copy()
            p[j] = (lo[j] if side < 0 else hi[j]) + side * 0.37 * ext
            extra.append(p)
    far = mid.copy()
    far[0] = 1e6
    Tc = np.vstack([Tc, extra, [far]])
    h0 = host_cell_size(Ts)
    h = {"one-cell": 2.0 * ext, "tenth": 0.1 * h0, "own": h0}[which]
    return Ts, Tc, G, grid(Ts, h)
