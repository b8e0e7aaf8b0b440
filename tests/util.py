"""Shared test helpers: seeded synthetic graphs (numpy), canonical forms, and a stub of the C library for the tests of the Python ->
C mapping."""
import contextlib
import ctypes

import numpy as np


def ba_graph(n, m, seed):
    """Barabasi-Albert graph (networkx-style repeated-endpoint list), returned as a
    symmetric, coalesced (2,E) int64 edge_index sorted by (col,row)."""
    rng = np.random.RandomState(seed)
    targets = list(range(m))
    rep = []
    src, dst = [], []
    for i in range(m, n):
        src.extend([i] * len(targets))
        dst.extend(targets)
        rep.extend(targets)
        rep.extend([i] * len(targets))
        chosen = set()
        while len(chosen) < m:
            chosen.add(rep[rng.randint(len(rep))])
        targets = sorted(chosen)
    a = np.array(src, dtype=np.int64)
    b = np.array(dst, dtype=np.int64)
    return symmetrize(a, b, n)


def symmetrize(a, b, n):
    r = np.concatenate([a, b])
    c = np.concatenate([b, a])
    key = np.unique(c * n + r)
    return np.stack([key % n, key // n]).astype(np.int64)


def clique(n):
    a, b = np.triu_indices(n, 1)
    return symmetrize(a.astype(np.int64), b.astype(np.int64), n)


def path(n):
    a = np.arange(n - 1, dtype=np.int64)
    return symmetrize(a, a + 1, n)


def star(n):
    a = np.zeros(n - 1, dtype=np.int64)
    return symmetrize(a, np.arange(1, n, dtype=np.int64), n)


def grid2d(h, w):
    idx = np.arange(h * w).reshape(h, w)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return symmetrize(a.astype(np.int64), b.astype(np.int64), h * w)


def sym_weights(edge_index, n, seed, lo=0.5, hi=1.5):
    """Tie-free symmetric weights: w(a,b) = w(b,a) drawn U(lo,hi) per undirected edge."""
    r, c = edge_index
    lo_id = np.minimum(r, c)
    hi_id = np.maximum(r, c)
    und = lo_id * n + hi_id
    uniq, inv = np.unique(und, return_inverse=True)
    rng = np.random.RandomState(seed)
    w = rng.uniform(lo, hi, size=uniq.shape[0])
    return w[inv]


def canonical(sc):
    """Rows sorted by (col,row): the edge-set view every caller consumes (L1 parity)."""
    sc = np.asarray(sc)
    if sc.shape[0] == 0:
        return sc
    order = np.lexsort((sc[:, 0], sc[:, 1]))
    return sc[order]


def introsort_killer(n):
    """Keys (distinct ints as float64) that drive libstdc++'s std::sort (threshold 16, median-of-3 to first, unguarded
    Hoare partition, depth limit 2*floor(log2 n)) into its heap-sort branch: McIlroy's adversary ("A Killer Adversary for
    Quicksort", 1999) run against a restatement of the introsort loop.  Returns (keys, hit_depth_limit)."""
    GAS = 1 << 60
    val = [GAS] * n
    state = {"nsolid": 0, "cand": 0}

    def less(x, y):   # x, y: item ids
        if val[x] == GAS and val[y] == GAS:
            if x == state["cand"]:
                val[x] = state["nsolid"]
            else:
                val[y] = state["nsolid"]
            state["nsolid"] += 1
        if val[x] == GAS:
            state["cand"] = x
        elif val[y] == GAS:
            state["cand"] = y
        return val[x] < val[y]

    a = list(range(n))
    depth0 = 2 * (n.bit_length() - 1)
    hit = False
    stack = [(0, n, depth0)]
    while stack:
        first, last, depth = stack.pop()
        while last - first > 16:
            if depth == 0:
                hit = True
                break
            depth -= 1
            ia, ib, ic = first + 1, first + (last - first) // 2, last - 1
            if less(a[ia], a[ib]):
                pick = ib if less(a[ib], a[ic]) else (ic if less(a[ia], a[ic]) else ia)
            elif less(a[ia], a[ic]):
                pick = ia
            elif less(a[ib], a[ic]):
                pick = ic
            else:
                pick = ib
            a[first], a[pick] = a[pick], a[first]
            pv = a[first]
            f, l = first + 1, last
            while True:
                while less(a[f], pv):
                    f += 1
                l -= 1
                while less(pv, a[l]):
                    l -= 1
                if not f < l:
                    break
                a[f], a[l] = a[l], a[f]
                f += 1
            stack.append((f, last, depth))
            last = f
    for i in range(n):
        if val[i] == GAS:
            val[i] = state["nsolid"]
            state["nsolid"] += 1
    return np.array(val, dtype=np.float64), hit


def wide_weights(edge_index, n, seed, decades):
    """Tie-free symmetric weights spread over many orders of magnitude: w(a,b) = w(b,a) = 10^u, u ~ U(-decades, decades) per
    undirected edge.  Eliminations then meet f close to 1 and new weights that round to <= 0 (the dead-entry rules) on small graphs."""
    r, c = edge_index
    und = np.minimum(r, c) * n + np.maximum(r, c)
    uniq, inv = np.unique(und, return_inverse=True)
    w = 10.0 ** np.random.RandomState(seed).uniform(-decades, decades, size=uniq.shape[0])
    assert np.unique(w).size == w.size
    return w[inv]


def assert_kernel(ops, expected, what=""):
    """The elimination kernel that produced the last call's rows (rlap_stats.elim_kernel: 0 none, 1 round kernel, 2 dataflow)."""
    st = ops.last_stats
    assert st["elim_kernel"] == expected, (f"{what}: elimination kernel {st['elim_kernel']}, expected {expected} "
                                           f"(retry_causes {st['retry_causes']:#x}, flow_abort {st['flow_abort']}, n_retries {st['n_retries']})")


def default_kernel(o_v, G, n_total):
    """The kernel the host's default rule picks for a call of G graphs (a views call: K * G) and n_total vertices
    (test_gpu_flow.py::test_default_kernel_choice pins the rule itself)."""
    return 2 if o_v == "random" and (G <= 2 or (G <= 64 and n_total >= 1024 * G)) else 1


def kernel_for(kernel, n, t):
    """What elim_kernel reports for a single graph of n vertices with num_remove t run on `kernel`: nothing runs when no vertex goes."""
    return kernel if min(t, n - 1) > 0 else 0


def i64_at(addr, count):
    """`count` int64 values read through an address a stubbed export was given."""
    return list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_int64))[:count])


def f64_at(addr, count):
    return list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_double))[:count])


class StubLib:
    """The C library without a GPU: `sigs` maps every export under test to the names of its positional arguments
    (include/rlap_hip.h); a call of one goes to export(name, {argument name: value}), which a test's subclass provides -- it records
    what it was given in `calls` and writes a result of its own.  The handle and arena calls around it answer as the library does."""

    def __init__(self, sigs, status=0):
        self.sigs = sigs
        self.calls = []
        self.status = status
        self.ws_needed = 1 << 12

    def rlap_create(self, out):
        out._obj.value = 0x1000
        return 0

    def rlap_destroy(self, h):
        return 0

    def rlap_set_rng_mode(self, h, mode):
        self.calls.append(("rlap_set_rng_mode", {"mode": mode}))
        return 0

    def rlap_workspace_query(self, h, E, n_total, G, symmetrize, ws_bytes, rng_entries):
        self.calls.append(("rlap_workspace_query", {"args": (E, n_total, G, symmetrize)}))
        ws_bytes._obj.value = 1 << 12
        rng_entries._obj.value = 1 << 10
        return 0

    def rlap_set_workspace(self, h, d_ws, ws_bytes, d_rng, rng_entries):
        self.calls.append(("rlap_set_workspace", {"ws_bytes": ws_bytes, "rng_entries": rng_entries}))
        return 0

    def rlap_workspace_needed(self, h, ws_bytes, rng_entries):
        self.calls.append(("rlap_workspace_needed", {}))
        ws_bytes._obj.value = self.ws_needed
        rng_entries._obj.value = 1 << 10
        return 0

    def __getattr__(self, name):
        if name == "sigs" or name not in self.sigs:
            raise AttributeError(name)
        return lambda *args: self.export(name, dict(zip(self.sigs[name].split(), args)))

    def export(self, name, a):
        raise NotImplementedError

    def exports(self):
        return [c for c in self.calls if c[0] in self.sigs]


def stub_ops(monkeypatch, stub):
    """rlap_amd.ops on `stub`: the device is the CPU, the handle the stub's, status strings are "status <rc>"."""
    import torch
    from rlap_amd import _lib, ops
    monkeypatch.setattr(ops, "_device_for", lambda t: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "device", contextlib.nullcontext)
    hobj = ops._Handle(stub, 0)
    monkeypatch.setattr(ops, "_handle_obj", lambda dev: (stub, hobj))
    monkeypatch.setattr(ops, "last_stats", None)
    monkeypatch.setattr(_lib, "status_string", lambda rc: f"status {rc}")   # (the message of a failed call, without the library)
    return stub
