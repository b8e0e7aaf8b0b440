"""Python host side of the augmentor: the reference's operator interface
(rlap/ops.py:7-63) on top of the C ABI of librlap_hip.so.

Same positional signature, same asserts, same return contract ((m,3) float64
[row, col, w], CPU tensor by default).  Differences, all deliberate:
  * inputs stay on the GPU (no `.cpu()` round trip, ops.py:47); CPU inputs are
    copied to the current HIP device -- there is no CPU compute path;
  * node ids are not squeezed through float32 (ops.py:47 promotes to f32 first,
    exact only below 2^24);
  * asymmetric input raises ValueError instead of exit(0) (factorizers.cc:19-22);
  * the randomness the reference takes from std::random_device is drawn from
    torch's RNG (or the keyword-only `perm` / `seed`), so runs are reproducible.
"""
from typing import Optional, Sequence, Tuple, Union
import ctypes
import threading
import warnings

import torch
from torch import Tensor

from . import _lib

O_V = {"random": 0, "degree": 1, "coarsen": 2}
O_N = {"asc": 0, "desc": 1, "random": 2}

# One handle (workspace + stream binding) per (device, host thread): the reference builds a fresh
# ApproximateCholesky per call (py_api_binder.cc:57), so calls from several Python threads must not share
# state.  ctypes releases the GIL during a call, so two threads really run side by side on their streams.
_tls = threading.local()
_timing = False
last_stats = None  # rlap_stats of the most recent call (dict), for benches/tests


class DataflowFallbackWarning(RuntimeWarning):
    """The dataflow elimination kernel (o_v="random") gave up inside a call (rlap_stats.flow_abort says why) and the call was
    repeated on the round kernel.  The rows are still the right ones; the warning says that the fast path did not produce them."""


class _Handle:
    """C-ABI handle plus the two torch tensors it works in: the per-call arena and the cached uniform table.  The library
    allocates nothing itself (rlap_set_workspace): like the reference's result tensor (py_api_binder.cc:42) the memory comes
    from torch's caching allocator, so the op runs inside a training loop that holds most of the device memory."""

    def __init__(self, lib, idx):
        self.lib = lib
        self.ptr = ctypes.c_void_p()
        self.ws = None
        self.rng = None
        with torch.cuda.device(idx):
            rc = lib.rlap_create(ctypes.byref(self.ptr))
        if rc != 0:
            raise RuntimeError(f"rlap_create failed: {_lib.status_string(rc)}")

    def fit(self, dev, ws_bytes: int, rng_entries: int):
        """Make the arena / table at least this large (grow-only, 12.5 % slack: no reallocation inside a size class)."""
        changed = False
        if self.ws is None or self.ws.numel() < ws_bytes:
            self.ws = None   # (released first: the allocator may hand the same block back, grown)
            self.ws = torch.empty(int(ws_bytes) + int(ws_bytes) // 8 + 4096, dtype=torch.uint8, device=dev)
            changed = True
        if self.rng is None or self.rng.numel() < rng_entries:
            self.rng = None
            self.rng = torch.empty(int(rng_entries) + int(rng_entries) // 8 + 1024, dtype=torch.float64, device=dev)
            changed = True
        if changed:
            rc = self.lib.rlap_set_workspace(self.ptr, self.ws.data_ptr(), self.ws.numel(), self.rng.data_ptr(), self.rng.numel())
            if rc != 0:
                _raise(rc)

    def __del__(self):
        try:
            if self.ptr:
                self.lib.rlap_destroy(self.ptr)
        except Exception:
            pass


def _device_for(t: Optional[Tensor]) -> torch.device:
    if t is not None and t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("rlap_amd needs a HIP device (MI355X); no GPU is visible and there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _handle_obj(device: torch.device):
    lib = _lib.load()
    idx = device.index if device.index is not None else torch.cuda.current_device()
    handles = getattr(_tls, "handles", None)
    if handles is None:
        handles = _tls.handles = {}
    hobj = handles.get(idx)
    if hobj is None:
        hobj = handles[idx] = _Handle(lib, idx)
    h = hobj.ptr
    lib.rlap_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream(idx).cuda_stream))
    lib.rlap_set_timing(h, 1 if _timing else 0)
    return lib, hobj


def _handle(device: torch.device):
    lib, hobj = _handle_obj(device)
    return lib, hobj.ptr


MODES = {"exact": 0, "frontier": 1}


def _set_mode(lib, h, mode: str):
    """`mode` of SURVEY 8(b): "exact" (default) draws the reference's one MT19937-64 stream in elimination order -- results equal
    the reference's; "frontier" draws counter-based uniforms keyed by (seed, vertex, position): the same distribution, bit-exact
    against the oracle run in that mode, not against the reference (include/rlap_hip.h::rlap_set_rng_mode)."""
    assert mode in MODES, f"mode must be one of {sorted(MODES)}"
    rc = lib.rlap_set_rng_mode(h, MODES[mode])
    if rc != 0:
        _raise(rc)


def _trim(out: torch.Tensor, rows: int) -> torch.Tensor:
    """The first `rows` rows of the (E,3) result buffer.  A view keeps the whole buffer alive, a copy costs a pass over the
    result (0.6 ms for the 1.5 GB of the 1024-graph batch): copy only when the view would pin more than a third on top."""
    res = out[:rows]
    if 4 * rows < 3 * out.shape[0]:
        res = res.clone()
    return res


def _run(hobj, dev, E: int, n_total: int, G: int, symmetrize: bool, call, st):
    """One op call inside torch-owned memory: size the arena for (E, n_total, G), call, and when the library reports
    that it wants more (a growth limit was met and the repeated attempt is of a larger size class) grow and call again."""
    lib = hobj.lib
    ws_b, rng_n = ctypes.c_size_t(0), ctypes.c_int64(0)
    if n_total is None:
        # num_nodes is found on the device inside the call: no bound is asked for up front (the only host-known one, 2 * E vertices,
        # is off by twice the mean degree -- gigabytes at ogbn-arxiv size, and RLAP_E_TOO_LARGE long before the true n is).  The call
        # itself says what it wants at the true n (RLAP_E_WORKSPACE, below) when the arena at hand is too small.
        hobj.fit(dev, 4096, 1 << 16)
    else:
        rc = lib.rlap_workspace_query(hobj.ptr, E, n_total, G, 1 if symmetrize else 0, ctypes.byref(ws_b), ctypes.byref(rng_n))
        if rc != 0:
            _raise(rc)
        hobj.fit(dev, ws_b.value, rng_n.value)
    retries, causes, abort = 0, 0, 0
    for _ in range(8):
        rc = call()
        retries += int(st.n_retries)
        causes |= int(st.retry_causes)
        abort = int(st.flow_abort) or abort
        if rc != _lib.E_WORKSPACE:
            break
        rc2 = lib.rlap_workspace_needed(hobj.ptr, ctypes.byref(ws_b), ctypes.byref(rng_n))
        if rc2 != 0:
            _raise(rc2)
        hobj.fit(dev, ws_b.value, rng_n.value)
    st.n_retries = retries
    st.retry_causes = causes
    st.flow_abort = abort
    if causes & _lib.RETRY_FLOW_GAVE_UP:
        # (bit 7, a reorder buffer too small, is a designed fall-back and stays quiet)
        warnings.warn(f"rlap: the dataflow elimination kernel gave up ({_lib.FLOW_ABORT_REASONS.get(abort, abort)}); "
                      "the call was repeated on the round kernel", DataflowFallbackWarning, stacklevel=4)
    return rc


def set_timing(enable: bool):
    """Fill the ms_* fields of `last_stats` with HIP-event timings (process-wide: every handle, every device)."""
    global _timing
    _timing = bool(enable)


def debug_set_limits(pool_factor: float = -1.0, log_factor: float = -1.0, rng_len: int = -1, scratch_entries: int = -1, device=None):
    """Test hook: tiny first-attempt workspace limits for the calling thread's handle, so that the
    overflow -> retry path of the C ABI runs (last_stats["n_retries"])."""
    dev = _device_for(None) if device is None else torch.device(device)
    lib, h = _handle(dev)
    rc = lib.rlap_debug_set_limits(h, float(pool_factor), float(log_factor), int(rng_len), int(scratch_entries))
    if rc != 0:
        _raise(rc)


def debug_set_flow_limits(reorder_cap: int = -1, device=None):
    """Test hook: entries of the dataflow kernel's reorder buffer for the first attempt of the calling thread's next call
    (negative = default), so that the fall-back to the round kernel runs (last_stats["retry_causes"] bit 7)."""
    dev = _device_for(None) if device is None else torch.device(device)
    lib, h = _handle(dev)
    rc = lib.rlap_debug_set_flow_limits(h, int(reorder_cap))
    if rc != 0:
        _raise(rc)


def debug_set_poison(byte: int = -1, device=None):
    """Debug aid: fill the workspace, the output buffer and the elimination kernel's LDS with `byte` before every attempt of
    the calling thread's next calls (negative = off); see include/rlap_hip.h."""
    dev = _device_for(None) if device is None else torch.device(device)
    lib, h = _handle(dev)
    rc = lib.rlap_debug_set_poison(h, int(byte))
    if rc != 0:
        _raise(rc)


def debug_set_jitter(quarter_us: int = 0, device=None):
    """Debug aid: waves of the elimination kernel sleep `quarter_us` x 0.25 us behind its barriers, a different subset each time
    (0 = off); see include/rlap_hip.h.  Results must not depend on it."""
    dev = _device_for(None) if device is None else torch.device(device)
    lib, h = _handle(dev)
    rc = lib.rlap_debug_set_jitter(h, int(quarter_us))
    if rc != 0:
        _raise(rc)


def _raise(rc: int):
    msg = _lib.status_string(rc)
    if rc in (1, 2, 3):
        raise ValueError(f"rlap: {msg}")
    raise RuntimeError(f"rlap: {msg} (status {rc})")


def _prep_edges(edge_index: Tensor, edge_weights: Optional[Tensor], dev: torch.device):
    assert edge_index.shape[0] == 2
    E = edge_index.shape[1]
    ei = edge_index.to(device=dev, dtype=torch.int64)
    row = ei[0].contiguous()
    col = ei[1].contiguous()
    w = None
    if edge_weights is not None:
        w = edge_weights.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()  # (1,E) or (E,)
        assert w.numel() == E, "edge_weights must have one entry per edge"
    return row, col, w, E


def _seed_from(seed: Optional[int]) -> int:
    if seed is None:
        return int(torch.randint(0, 2**62, (1,)).item())
    return int(seed) & (2**64 - 1)


def _eliminate(export: str, args: tuple, edge_index: Tensor, edge_weights: Optional[Tensor], o_v: str, o_n: str, perm, seed,
               mode: str, return_device, *, n: Optional[int], G: int = 1, K: int = 1, D: int = 1, symmetrize: bool = False,
               rows_only: bool = False, outs: tuple = ()):
    """The body every elimination entry point shares: one call of the C export `export`, whose own arguments are `args` (those
    between E and o_v) and `outs` (outputs between the row offsets and the stats).  The call is K views of a batch of G graphs of
    n vertices in all (None: found by the call), D nested depths each, of the input as given or with both directions of every edge
    (symmetrize).  That sizes the output (D*K*E rows, twice that for symmetrize: an elimination never adds entries), the row
    offsets (D*K*G+1, or with rows_only the one row count the export writes), the arena (_run) and `perm` (K*n entries).
    Returns (sc_edge_info, ptr): ptr the row offsets, a c_int64 with rows_only."""
    assert edge_index.shape[0] == 2
    assert o_v in ["random", "degree", "coarsen"]
    assert o_n in ["asc", "desc", "random"]
    global last_stats
    dev = _device_for(edge_index)
    lib, hobj = _handle_obj(dev)
    _set_mode(lib, hobj.ptr, mode)
    fn = getattr(lib, export)
    with torch.cuda.device(dev):
        row, col, w, E = _prep_edges(edge_index, edge_weights, dev)
        d_perm = None
        if o_v == "random" and perm is not None:
            d_perm = perm.to(device=dev, dtype=torch.int64).contiguous()
            assert n is not None and d_perm.numel() == K * n, "perm must hold views * num_nodes entries"
        # perm None: the reference shuffles 0..n-1 with std::random_device (preconditioner.cc:594-596); here every node_id vector is
        # drawn on the device from `seed` by the C ABI's keyed shuffle (ONE meaning of `seed` in this module)
        shuffle_seed = _seed_from(seed) if (o_n == "random" or o_v != "degree" or mode == "frontier") else 0
        out = torch.empty((max(D * K * (2 if symmetrize else 1) * E, 1), 3), dtype=torch.float64, device=dev)
        ptr = ctypes.c_int64(0) if rows_only else torch.zeros(D * K * G + 1, dtype=torch.int64)
        st = _lib.Stats()
        # (views: the arena of a batched call on the K-fold union, include/rlap_hip.h)
        rc = _run(hobj, dev, K * E, None if n is None else K * n, K * G, symmetrize, lambda: fn(
            hobj.ptr, row.data_ptr(), col.data_ptr(), w.data_ptr() if w is not None else None, E, *args, O_V[o_v], O_N[o_n],
            d_perm.data_ptr() if d_perm is not None else None, shuffle_seed, out.data_ptr(), out.shape[0],
            ctypes.byref(ptr) if rows_only else ptr.data_ptr(), *outs, ctypes.byref(st)), st)
        if rc != 0:
            _raise(rc)
        last_stats = st.as_dict()
        res = _trim(out, ptr.value if rows_only else int(ptr[-1]))
    if return_device is not None and return_device != "same":
        res = res.to(return_device)
    return res, ptr


def approximate_cholesky(
    edge_index: Tensor,
    edge_weights: Optional[Tensor],
    num_nodes: int,
    num_remove: int,
    o_v: str,
    o_n: str,
    *,
    perm: Optional[Tensor] = None,
    seed: Optional[int] = None,
    return_device: Optional[Union[str, torch.device]] = "cpu",
    mode: str = "exact",
) -> Tensor:
    """Randomized Schur complement of the graph Laplacian (reference: rlap/ops.py:7-58).

    Keyword-only extras: `perm` (o_v="random": the elimination order vector, popped
    from the back, preconditioner.cc:588-613), `seed` (draws `perm` / the neighbour
    shuffles reproducibly), `return_device` ("cpu" as the reference, None/"same" to
    keep the result on the GPU).
    """
    n = int(num_nodes)
    res, _ = _eliminate("rlap_approx_chol", (n, int(num_remove)), edge_index, edge_weights, o_v, o_n, perm, seed, mode,
                        return_device, n=n, rows_only=True)
    return res


def approximate_cholesky_from_edges(
    edge_index: Tensor,
    edge_weights: Optional[Tensor] = None,
    num_nodes: Optional[int] = None,
    num_remove: Optional[int] = None,
    o_v: str = "random",
    o_n: str = "asc",
    *,
    remove_frac: float = 0.5,
    symmetrize: bool = True,
    perm: Optional[Tensor] = None,
    seed: Optional[int] = None,
    return_device: Optional[Union[str, torch.device]] = None,
    mode: str = "exact",
) -> Tuple[Tensor, int]:
    """The op with the step before it fused into its COO->CSR kernels:
    `to_undirected` + coalesce (scripts/node_shared.py:326-327) when `symmetrize`, and
    `num_nodes = edge_index.max() + 1`, `num_remove = int(remove_frac * num_nodes)`
    (scripts/augmentor_benchmarks.py:77-78) when they are None -- found on the device, without a
    torch reduction + `.item()`.  Returns (sc_edge_info on the device, num_nodes)."""
    n = -1 if num_nodes is None else int(num_nodes)   # (n < 0: found on the device)
    t = -1 if num_remove is None else int(num_remove)
    nn = ctypes.c_int64(0)
    res, _ = _eliminate("rlap_approx_chol_from_edges", (n, t, float(remove_frac), 1 if symmetrize else 0), edge_index, edge_weights,
                        o_v, o_n, perm, seed, mode, return_device, n=n if n >= 0 else None, symmetrize=bool(symmetrize),
                        rows_only=True, outs=(ctypes.byref(nn),))
    return res, int(nn.value)


def approximate_cholesky_batched(
    edge_index: Tensor,
    edge_weights: Optional[Tensor],
    node_ptr: Union[Tensor, Sequence[int]],
    num_remove: Union[Tensor, Sequence[int]],
    o_v: str,
    o_n: str,
    *,
    perm: Optional[Tensor] = None,
    seed: Optional[int] = None,
    return_device: Optional[Union[str, torch.device]] = None,
    mode: str = "exact",
) -> Tuple[Tensor, Tensor]:
    """Batched-graph mode: graph g owns node ids [node_ptr[g], node_ptr[g+1]).

    Every graph is eliminated independently -- what G separate reference calls would
    return, concatenated, with global node ids: graph g's rows equal
    `approximate_cholesky(graph g, ..., perm=perm[g], seed=seed + g)` shifted by node_ptr[g].
    Returns (sc_edge_info, row_ptr[G+1]).  `perm` concatenates per-graph permutations of LOCAL ids.
    """
    np_ = torch.as_tensor(node_ptr, dtype=torch.int64).cpu().contiguous()
    nr_ = torch.as_tensor(num_remove, dtype=torch.int64).cpu().contiguous()
    G = np_.numel() - 1
    assert nr_.numel() == G
    return _eliminate("rlap_approx_chol_batched", (G, np_.data_ptr(), nr_.data_ptr()), edge_index, edge_weights, o_v, o_n, perm,
                      seed, mode, return_device, n=int(np_[-1]), G=G)


def approximate_cholesky_views(
    edge_index: Tensor,
    edge_weights: Optional[Tensor],
    num_nodes: int,
    num_remove: Union[int, Tensor, Sequence[int], Sequence[Sequence[int]]],
    o_v: str,
    o_n: str,
    *,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    perm: Optional[Tensor] = None,
    seed: Optional[int] = None,
    return_device: Optional[Union[str, torch.device]] = None,
    mode: str = "exact",
) -> Tuple[Tensor, Tensor]:
    """K independent Schur complements ("views") of one input in one call -- the two augmentations of a graph-contrastive
    training step (scripts/node_shared.py:260-262) without K setups.

    The input is one graph of `num_nodes` vertices, or with `node_ptr` a batch of G graphs as in approximate_cholesky_batched
    (then `num_nodes` must equal node_ptr[-1]).  `num_remove` gives K: an int is K = 1, a length-K sequence one value per view
    (every graph of the view), a (K, G) tensor or nested sequence one value per (view, graph).
    Returns (sc_edge_info, ptr[K*G+1]): rows grouped view-major (all graphs of view 0, then view 1, ...), node ids in the
    INPUT's id space.  (view k, graph g) equals `approximate_cholesky(graph g, ..., perm=perm slice (k, g), seed=seed + k*G + g)`
    -- graph k*G + g of approximate_cholesky_batched on the K-fold disjoint union, ids shifted back.  `perm` (o_v="random") holds
    K*N entries: per view, per graph, a permutation of local ids.

    In mode "exact", o_v="degree" with o_n "asc" or "desc" draws no seeded randomness (the reference uses a default-seeded
    std::mt19937_64, preconditioner.cc:356), so two views with equal num_remove are identical -- as in the reference.
    mode="frontier" gives distinct samples.
    """
    n = int(num_nodes)
    np_ = torch.as_tensor([0, n] if node_ptr is None else node_ptr, dtype=torch.int64).cpu().contiguous()
    G = np_.numel() - 1
    assert G >= 1 and int(np_[-1]) == n, "node_ptr[-1] must equal num_nodes"
    nr_ = torch.as_tensor(num_remove, dtype=torch.int64).cpu()
    if nr_.dim() == 0:
        nr_ = nr_.reshape(1, 1).expand(1, G)
    elif nr_.dim() == 1:
        nr_ = nr_.reshape(-1, 1).expand(nr_.numel(), G)
    assert nr_.dim() == 2 and nr_.shape[1] == G and nr_.shape[0] >= 1, "num_remove: an int, K values, or (K, G)"
    K = int(nr_.shape[0])
    nr_ = nr_.contiguous()
    return _eliminate("rlap_approx_chol_views", (G, np_.data_ptr(), K, nr_.data_ptr()), edge_index, edge_weights, o_v, o_n, perm,
                      seed, mode, return_device, n=n, G=G, K=K)


def _depths_list(num_remove) -> list:
    """num_remove of approximate_cholesky_depths as a list of ints: non-empty, non-decreasing (checked here, before any device
    or library call)."""
    if isinstance(num_remove, Tensor):
        if num_remove.dtype.is_floating_point or num_remove.dtype == torch.bool or num_remove.dim() > 1:
            raise ValueError("num_remove: a sequence of integers")
        vals = [int(v) for v in num_remove.reshape(-1).tolist()]
    else:
        try:
            vals = list(num_remove)
        except TypeError:
            raise ValueError("num_remove: a sequence of integers, one depth per snapshot") from None
        for v in vals:
            if isinstance(v, bool) or not hasattr(v, "__index__"):   # (ints and numpy integers; not floats, not bools)
                raise ValueError(f"num_remove: integers only, got {v!r}")
        vals = [v.__index__() for v in vals]
    if not vals:
        raise ValueError("num_remove: at least one depth")
    if any(b < a for a, b in zip(vals, vals[1:])):
        raise ValueError(f"num_remove must be non-decreasing, got {vals}")
    return vals


def _int_tensor(x, what: str) -> Tensor:
    """`x` (a tensor, or a possibly nested sequence of ints / numpy integers) as an int64 CPU tensor; ValueError for floats, bools,
    strings or ragged nesting -- torch.as_tensor would convert some of them silently."""
    if isinstance(x, Tensor):
        if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
            raise ValueError(f"{what}: integers only")
        return x.detach().to(device="cpu", dtype=torch.int64)

    def bad(v) -> bool:
        if isinstance(v, (bool, str, bytes, float)):
            return True
        if hasattr(v, "__index__"):
            return False
        try:
            return any(bad(u) for u in v)
        except TypeError:
            return True
    if bad(x):
        raise ValueError(f"{what}: integers only")
    try:
        return torch.as_tensor(x, dtype=torch.int64)
    except (TypeError, ValueError, RuntimeError, OverflowError):
        raise ValueError(f"{what}: a regular array of integers") from None


def _depths_table(num_remove, num_nodes: int, node_ptr, views) -> Tuple[Tensor, Tensor, int, int]:
    """Arguments of a batched / views depths call, checked before any device or library call: (node_ptr, table[D, K*G], K, G),
    table[d, k*G + g] = depth d of (view k, graph g).  num_remove is (D,), every (view, graph) alike, or (D, K, G)."""
    if isinstance(views, bool) or not hasattr(views, "__index__") or views.__index__() < 1:
        raise ValueError(f"views: a positive integer, got {views!r}")
    K = views.__index__()
    n = int(num_nodes)
    np_ = torch.tensor([0, n], dtype=torch.int64) if node_ptr is None else _int_tensor(node_ptr, "node_ptr")
    if np_.dim() != 1 or np_.numel() < 2 or int(np_[0]) != 0 or bool((np_[1:] < np_[:-1]).any()):
        raise ValueError("node_ptr: non-decreasing offsets starting at 0, at least one graph")
    if int(np_[-1]) != n:
        raise ValueError(f"node_ptr[-1] ({int(np_[-1])}) must equal num_nodes ({n})")
    G = np_.numel() - 1
    t = _int_tensor(num_remove, "num_remove")
    if t.dim() == 1 and t.numel() >= 1:
        t = t.reshape(-1, 1, 1).expand(t.numel(), K, G)
    elif t.dim() != 3 or tuple(t.shape[1:]) != (K, G) or t.shape[0] < 1:
        raise ValueError(f"num_remove: (D,) or (D, K={K}, G={G}) integers, got shape {tuple(t.shape)}")
    t = t.reshape(t.shape[0], K * G).contiguous()
    if bool((t[1:] < t[:-1]).any()):
        raise ValueError("num_remove must be non-decreasing down every (view, graph) column")
    return np_.contiguous(), t, K, G


def _one_graph_depths(num_remove, node_ptr, views) -> bool:
    """The call of a depths list for one graph, one view: today's path through rlap_approx_chol_depths."""
    if node_ptr is not None or isinstance(views, bool) or not hasattr(views, "__index__") or views.__index__() != 1:
        return False
    if isinstance(num_remove, Tensor):
        return num_remove.dim() <= 1
    try:
        return torch.as_tensor(num_remove).dim() <= 1
    except Exception:
        return True   # (ragged or not numeric: _depths_list says what is wrong)


def approximate_cholesky_depths(
    edge_index: Tensor,
    edge_weights: Optional[Tensor],
    num_nodes: int,
    num_remove: Sequence[int],
    o_v: str,
    o_n: str,
    *,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    views: int = 1,
    perm: Optional[Tensor] = None,
    seed: Optional[int] = None,
    return_device: Optional[Union[str, torch.device]] = None,
    mode: str = "exact",
) -> Tuple[Tensor, Tensor]:
    """K nested Schur complements ("depths") of one graph from ONE elimination -- the sweep over the removed fraction of the
    reference's analysis scripts (scripts/rlap_ppr_edge_plots.py:37, scripts/rlap_vc_spectral.py:14-58) without K calls.

    `num_remove` is a non-decreasing sequence t_0 <= ... <= t_{K-1} (zero and repeated values allowed; each value is clamped to
    num_nodes - 1 as in approximate_cholesky).  Returns (sc_edge_info, ptr[K+1]): snapshot k is rows [ptr[k], ptr[k+1]) and equals
    `approximate_cholesky(..., num_remove=t_k, perm=perm, seed=seed, mode=mode)` -- indices, row order and weights -- because the
    elimination to t_k passes through exactly the state a call with a smaller num_remove stops in.  Node ids stay in the input's
    space (no relabel between depths).  The elimination runs once, in segments [t_{k-1}, t_k), each followed by the output pass
    of its snapshot.

    Batches and views: `node_ptr` (a batch of G graphs, as in approximate_cholesky_batched) and `views` (K independent views, as
    in approximate_cholesky_views) take the depths of every (view, graph) from one elimination of the K-fold union.  Then
    `num_remove` is (D,), the same depths for every (view, graph), or a (D, K, G) tensor / nested sequence, non-decreasing down
    every (view, graph) column.  Returns (sc_edge_info, ptr[D*K*G+1]): rows depth-major, then view, then graph; snapshot
    (d, k, g) is rows [ptr[(d*K + k)*G + g], ptr[(d*K + k)*G + g + 1]) and equals depth row d of
    `approximate_cholesky_views(..., num_remove=t[d], node_ptr=node_ptr)`.  `perm` (o_v="random") then holds K*N entries laid
    out as for the views call; every depth uses it.
    """
    if not _one_graph_depths(num_remove, node_ptr, views):
        return _depths_views(edge_index, edge_weights, num_nodes, num_remove, o_v, o_n, node_ptr, views, perm, seed, return_device, mode)
    n = int(num_nodes)
    nr_ = torch.tensor(_depths_list(num_remove), dtype=torch.int64)
    D = nr_.numel()
    return _eliminate("rlap_approx_chol_depths", (n, D, nr_.data_ptr()), edge_index, edge_weights, o_v, o_n, perm, seed, mode,
                      return_device, n=n, D=D)


def _depths_views(edge_index, edge_weights, num_nodes, num_remove, o_v, o_n, node_ptr, views, perm, seed, return_device, mode):
    """approximate_cholesky_depths with `node_ptr` and / or `views`: one rlap_approx_chol_views_depths call."""
    n = int(num_nodes)
    np_, nr_, K, G = _depths_table(num_remove, n, node_ptr, views)
    D = int(nr_.shape[0])
    return _eliminate("rlap_approx_chol_views_depths", (G, np_.data_ptr(), K, D, nr_.data_ptr()), edge_index, edge_weights, o_v, o_n,
                      perm, seed, mode, return_device, n=n, G=G, K=K, D=D)


SNAPSHOT_MAX_ITER = 1024   # bound of max_iter (include/rlap_hip.h::rlap_snapshot_stats)


def _ptr_table(x, what: str, first: int, last: Optional[int]) -> Tensor:
    """A 1-D int64 CPU offset table: at least two entries, x[0] == first, non-decreasing, x[-1] == last (when given)."""
    t = _int_tensor(x, what)
    if t.dim() != 1 or t.numel() < 2:
        raise ValueError(f"{what}: a 1-D table of at least two offsets")
    if int(t[0]) != first or bool((t[1:] < t[:-1]).any()):
        raise ValueError(f"{what}: non-decreasing offsets starting at {first}")
    if last is not None and int(t[-1]) != last:
        raise ValueError(f"{what}[-1] ({int(t[-1])}) must equal {last}")
    return t.contiguous()


def _num_nodes(num_nodes) -> int:
    if isinstance(num_nodes, bool) or not hasattr(num_nodes, "__index__") or num_nodes.__index__() < 0:
        raise ValueError(f"num_nodes: a non-negative integer, got {num_nodes!r}")
    return num_nodes.__index__()


def _snapshot_tables(sc: Tensor, ptr, num_nodes: int, node_ptr) -> Tuple[Tensor, Optional[Tensor]]:
    """Host-side checks every snapshot entry point makes before anything is launched: (ptr, node_ptr) as int64 CPU tensors."""
    if not isinstance(sc, Tensor) or sc.dim() != 2 or sc.shape[1] != 3:
        raise ValueError("sc: an (m, 3) tensor of rows [row, col, w]")
    n = _num_nodes(num_nodes)
    p = _ptr_table(ptr, "ptr", 0, int(sc.shape[0]))
    S = p.numel() - 1
    np_ = None
    if node_ptr is not None:
        np_ = _ptr_table(node_ptr, "node_ptr", 0, n)
        G = np_.numel() - 1
        if S % G != 0:
            raise ValueError(f"node_ptr has {G} graphs, which does not divide the {S} segments of ptr")
    return p, np_


def _graphs(np_: Optional[Tensor]) -> int:
    return np_.numel() - 1 if np_ is not None else 1


def _snapshot_call(export: str, info_cls, x: Tensor, p: Tensor, np_: Optional[Tensor], n: int, tail: tuple, extra_msg: Optional[str] = None,
                   grouped: bool = True, accept: tuple = ()):
    """The call every snapshot entry point makes: the C export `export` on the rows `x` (float64, on the device), the tables p /
    np_ moved there, G and S derived from them, then the export's own arguments `tail` and an `info_cls` for its report.  Statuses
    1, 2, 3 (with `extra_msg` appended to 3) and, where the layout is checked (`grouped`), RLAP_E_NOT_GROUPED raise ValueError, the
    others RuntimeError; a status in `accept` is the caller's to handle.  Sets `last_stats` and returns the info struct."""
    global last_stats
    dev = x.device
    lib, hobj = _handle_obj(dev)
    fn = getattr(lib, export)
    S, G, m = p.numel() - 1, _graphs(np_), int(x.shape[0])
    d_ptr = p.to(dev)
    d_np = np_.to(dev) if np_ is not None else None
    info = info_cls()
    st = _lib.Stats()
    rc = _run(hobj, dev, m, None, G, False, lambda: fn(
        hobj.ptr, x.data_ptr() if m else None, m, d_ptr.data_ptr(), S, d_np.data_ptr() if d_np is not None else None, G, n,
        *tail, ctypes.byref(info)), st)
    if rc in accept:
        return info
    if rc in (1, 2, 3) or (grouped and rc == _lib.E_NOT_GROUPED):
        raise ValueError(f"rlap: {_lib.status_string(rc)}" + (extra_msg if rc == 3 and extra_msg else ""))
    if rc != 0:
        _raise(rc)
    last_stats = info.as_dict()
    return info


def _device_call(export: str, info_cls, dev, G: int, tail: tuple):
    """The call of the readout, the fused losses and the probe: the C export `export` on the library's device `dev` with the
    arguments `tail` behind the handle and an `info_cls` for its report.  Statuses 1, 2, 3 raise ValueError (with the report's
    `detail`, where it has one), the others RuntimeError.  Sets `last_stats` and returns the info struct."""
    global last_stats
    lib, hobj = _handle_obj(dev)
    fn = getattr(lib, export)
    info = info_cls()
    st = _lib.Stats()
    rc = _run(hobj, dev, 0, None, G, False, lambda: fn(hobj.ptr, *tail, ctypes.byref(info)), st)
    if rc in (1, 2, 3):
        raise ValueError(f"rlap: {_lib.status_string(rc)}" + (f" (detail {info.detail})" if hasattr(info, "detail") else ""))
    if rc != 0:
        _raise(rc)
    last_stats = info.as_dict()
    return info


def _upstream(g: Tensor, dev) -> Tensor:
    """The upstream gradient of a scalar loss as the backward exports read it: one float64 on the library's device."""
    return g.detach().to(device=dev, dtype=torch.float64).reshape(1).contiguous()


def snapshot_stats(
    sc: Tensor,
    ptr: Union[Tensor, Sequence[int]],
    num_nodes: int,
    *,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    weighted: bool = False,
    tol: float = 1e-10,
    max_iter: int = 1000,
) -> dict:
    """Per-snapshot statistics of a result of the calls above -- what scripts/rlap_vc_spectral.py:14-55 (get_rlap_sc_stats)
    records for every snapshot, computed on the device for all snapshots at once and without a dense matrix.

    `sc` is an (m, 3) [row, col, w] result and `ptr` its S+1 row offsets: segment s is rows [ptr[s], ptr[s+1]).  Id ranges: with
    node_ptr=None every id lies in [0, num_nodes) (single, views and depths results); with `node_ptr` (G+1 offsets, G dividing S)
    segment s is graph g = s % G and its ids lie in [node_ptr[g], node_ptr[g+1]) -- batched (g), views (k, g) and depths (d, k, g)
    results all put the graph index fastest.

    Returns a dict of (S,) tensors on sc's device:
      nodes      : distinct ids in the segment's rows, torch.unique(sc[ptr[s]:ptr[s+1], :2]).numel()  (num_unique_nodes)
      rows       : ptr[s+1] - ptr[s]                                                                    (num_edges)
      lambda_max : the largest eigenvalue of the segment's symmetric adjacency A, unweighted (unit entries, as to_dense_adj without
                   edge_attr) or with `weighted` the rows' weights; 0 for a segment without rows.  For A >= 0 (Perron-Frobenius)
                   it is the spectral radius and the largest singular value, the script's max_sv without svd_lowrank's estimate
      iters      : Lanczos steps taken (float64 plain three-term recurrence from the normalised all-ones vector on the segment's
                   ids; the largest eigenvalue theta of T_j found by Sturm bisection every 4 steps)
      converged  : whether beta_j |y_j| <= tol * theta (some eigenvalue of A lies within tol * theta of theta) held within max_iter
    The same input gives the same bits.  `sc` and `ptr` are only read; the scratch is the handle's arena, so the call does not
    change later results of any other.  A column whose rows are not contiguous within its segment, a row id without a column, or
    an id outside its segment's range raise ValueError.  `last_stats` then holds what the call did (rlap_snapshot_info).
    """
    p, np_ = _snapshot_tables(sc, ptr, num_nodes, node_ptr)
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not (0.0 < float(tol) < float("inf")):
        raise ValueError(f"tol: a positive number, got {tol!r}")
    if isinstance(max_iter, bool) or not hasattr(max_iter, "__index__") or not 1 <= max_iter.__index__() <= SNAPSHOT_MAX_ITER:
        raise ValueError(f"max_iter: an integer in [1, {SNAPSHOT_MAX_ITER}], got {max_iter!r}")
    S = p.numel() - 1
    dev = _device_for(sc)
    with torch.cuda.device(dev):
        x = sc.to(device=dev, dtype=torch.float64).contiguous()
        nodes = torch.empty(S, dtype=torch.int64, device=dev)
        lam = torch.empty(S, dtype=torch.float64, device=dev)
        iters = torch.empty(S, dtype=torch.int32, device=dev)
        conv = torch.empty(S, dtype=torch.int32, device=dev)
        _snapshot_call("rlap_snapshot_stats", _lib.SnapshotInfo, x, p, np_, int(num_nodes),
                       (1 if weighted else 0, float(tol), int(max_iter), nodes.data_ptr(), lam.data_ptr(), iters.data_ptr(), conv.data_ptr()))
        rows = (p[1:] - p[:-1]).to(dev)
    return {"nodes": nodes, "rows": rows, "lambda_max": lam, "iters": iters, "converged": conv.bool()}


PPR_MAX_STEPS = 4096   # cap on the Chebyshev steps K (rlap_amd/csrc/rlap_cheb.h::MAX_STEPS)
PPR_FIRST_CAP_PER_ROW = 16   # first output capacity of a PPR call: max(16 rows per input row + 64, PPR_FIRST_CAP_MIN), at most
PPR_FIRST_CAP_MIN = 1 << 22  # S * min(num_nodes, m)^2 (every pair of every segment); one retry with the exact count beyond


def ppr_steps(alpha: float, tol: float) -> int:
    """K = min{K >= 0 : T_K(1/(1-alpha)) >= 1/tol}, T_K by its three-term recurrence (the arithmetic of rlap_cheb.h::steps), or -1
    when K would exceed PPR_MAX_STEPS.  After K Chebyshev steps every entry of S lies within tol of exact."""
    mu, goal = 1.0 / (1.0 - float(alpha)), 1.0 / float(tol)
    if 1.0 >= goal:
        return 0
    tp, t = 1.0, mu
    for k in range(1, PPR_MAX_STEPS + 1):
        if t >= goal:
            return k
        tp, t = t, 2.0 * mu * t - tp
    return -1


def _real(x, what: str, lo: float, hi: float, lo_open: bool = True) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise ValueError(f"{what}: a number, got {x!r}")
    v = float(x)
    if not (v > lo if lo_open else v >= lo) or not v < hi:
        raise ValueError(f"{what}: must lie in ({lo}, {hi}), got {x!r}")
    return v


def _ppr_params(alpha, eps, tol) -> Tuple[float, float, float, int]:
    """Host-side checks of the PPR parameters, made before anything is launched."""
    a = _real(alpha, "alpha", 0.0, 1.0)
    e = _real(eps, "eps", 0.0, float("inf"))
    t = _real(tol, "tol", 0.0, float("inf"))
    K = ppr_steps(a, t)
    if K < 0:
        raise ValueError(f"alpha={a!r}, tol={t!r} need more than {PPR_MAX_STEPS} Chebyshev steps (T_K(1/(1-alpha)) >= 1/tol)")
    return a, e, t, K


def _ppr_call(x: Tensor, p: Tensor, np_: Optional[Tensor], n: int, alpha: float, eps: float, tol: float, flags: int) -> Tuple[Tensor, Tensor]:
    """One rlap_snapshot_ppr call inside torch-owned memory: the first output capacity is max(16 m + 64, 2^22) rows, at most
    S min(n, m)^2; when the kept entries exceed it the call writes nothing and reports the count, and is made once more with
    exactly that many."""
    global last_stats
    S, m, dev = p.numel() - 1, int(x.shape[0]), x.device
    cap = first_cap = min(S * min(n, m) ** 2, max(PPR_FIRST_CAP_PER_ROW * m + 64, PPR_FIRST_CAP_MIN))
    for retries in (0, 1):
        out = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        pptr = torch.empty(S + 1, dtype=torch.int64, device=dev)
        info = _snapshot_call("rlap_snapshot_ppr", _lib.PprInfo, x, p, np_, n,
                              (alpha, eps, tol, flags, out.data_ptr() if cap else None, cap, pptr.data_ptr()),
                              extra_msg=" (or a weight is <= 0)", accept=(_lib.E_OUT_CAPACITY,) if retries == 0 else ())
        P = int(info.rows_needed)
        if P <= cap:   # (more than the capacity: RLAP_E_OUT_CAPACITY, accepted on the first attempt only)
            break
        cap = P
    last_stats = dict(info.as_dict(), output_retries=retries, first_cap=first_cap)
    return _trim(out, P), pptr


def snapshot_ppr(
    sc: Tensor,
    ptr: Union[Tensor, Sequence[int]],
    num_nodes: int,
    *,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    alpha: float = 0.2,
    eps: float = 1e-4,
    tol: float = 1e-10,
    weighted: bool = True,
    add_self_loop: bool = False,
    normalize_out: bool = True,
) -> Tuple[Tensor, Tensor]:
    """Personalised-PageRank diffusion of every snapshot of a result of the calls above, on the device and without a dense matrix --
    rLapPPRDiffusion's compute_ppr (PyGCL: transition_matrix('sym'), diffusion_matrix_exact('ppr'), sparsify_dense('threshold'),
    transition_matrix('sym')) for all snapshots of one call.  `sc`, `ptr`, `num_nodes` and `node_ptr` as for snapshot_stats.

    For snapshot s with distinct ids V_s and symmetric adjacency A (the rows' weights, or unit entries with weighted=False; duplicate
    rows summed; A + I with add_self_loop), d = A 1:
        S = alpha (I - (1 - alpha) D^-1/2 A D^-1/2)^-1,  entries S_ij >= eps kept,  normalize_out: D_S^-1/2 S D_S^-1/2 (D_S: row sums)
    Returns (out (P, 3) float64 rows [i, j, value] in the input's id space, pptr (S+1,) int64), both on sc's device: segment s is rows
    [pptr[s], pptr[s+1]) in row-major order (ascending i, then j) -- the order of adapters.compute_ppr's nonzero() on the relabelled
    snapshot.  S comes from K fixed Chebyshev steps, K = ppr_steps(alpha, tol) (35 for the defaults): every entry lies within `tol`
    of exact before normalisation, so a keep decision can differ from the exact matrix only where |S_ij - eps| <= tol.  The result is
    exactly symmetric, the same input gives the same bits, and segment s equals the same call on that segment alone, bit for bit.

    alpha outside (0, 1), eps <= 0, tol <= 0, more than PPR_MAX_STEPS steps, malformed tables, a column not contiguous within its
    segment, a row id without a column, an id out of range, or (weighted) a weight <= 0 raise ValueError.  `last_stats` then holds
    what the call did (rlap_ppr_info: steps, small / large tiles, groups, launches, rows_needed, arena_bytes, host_syncs) and
    `output_retries` (1 when the first capacity guess was short).
    """
    p, np_ = _snapshot_tables(sc, ptr, num_nodes, node_ptr)
    alpha, eps, tol, _ = _ppr_params(alpha, eps, tol)
    if weighted and not sc.is_cuda and sc.shape[0] and not bool((sc[:, 2] > 0).all() and torch.isfinite(sc[:, 2]).all()):
        raise ValueError("sc: every weight must be > 0 (the spectral bound of the iteration needs A >= 0)")
    dev = _device_for(sc)
    flags = ((_lib.PPR_WEIGHTED if weighted else 0) | (_lib.PPR_SELF_LOOP if add_self_loop else 0)
             | (_lib.PPR_NORMALIZE if normalize_out else 0))
    with torch.cuda.device(dev):
        x = sc.to(device=dev, dtype=torch.float64).contiguous()
        return _ppr_call(x, p, np_, int(num_nodes), alpha, eps, tol, flags)


def _diffusion_input(edge_index: Tensor, edge_weights: Optional[Tensor], num_nodes: int, node_ptr) -> Tuple[Tensor, Tensor, Optional[Tensor], int]:
    """What ppr_diffusion and markov_diffusion make of a plain undirected edge list before their call: (sc, ptr, node_ptr, n) with
    sc the (m, 3) float64 rows on the device, grouped by column with a stable sort by (col, row), rows of weight 0 dropped, duplicates
    summed in input order, symmetry checked, and a row (i, i, 0) for every id without edges.  With `node_ptr` (a batch's contiguous
    id ranges) every graph is a segment of its own -- ptr holds its rows, found by searchsorted of the column ids -- and a row whose
    two ends lie in different graphs raises ValueError; without it the list is one segment."""
    n = _num_nodes(num_nodes)
    if not isinstance(edge_index, Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index: a (2, E) tensor")
    E = int(edge_index.shape[1])
    w = edge_weights
    if w is not None:
        w = w.reshape(-1)
        if w.numel() != E:
            raise ValueError("edge_weights must have one entry per edge")
        if E and not bool((w >= 0).all()):
            raise ValueError("edge_weights: a weight is negative (or not a number)")
    np_ = _ptr_table(node_ptr, "node_ptr", 0, n) if node_ptr is not None else None
    if E and not edge_index.is_cuda and (int(edge_index.min()) < 0 or int(edge_index.max()) >= n):
        raise ValueError(f"edge_index: ids must lie in [0, {n})")
    dev = _device_for(edge_index)
    with torch.cuda.device(dev):
        ei = edge_index.to(device=dev, dtype=torch.int64).contiguous()
        w = torch.ones(E, dtype=torch.float64, device=dev) if w is None else w.to(device=dev, dtype=torch.float64)
        if E and (int(ei.min()) < 0 or int(ei.max()) >= n):
            raise ValueError(f"edge_index: ids must lie in [0, {n})")
        if np_ is not None and E:
            bounds = np_[1:].to(dev)
            if not torch.equal(torch.searchsorted(bounds, ei[0], right=True), torch.searchsorted(bounds, ei[1], right=True)):
                raise ValueError("edge_index: a row joins two graphs of node_ptr")
        keep = w != 0
        ei, w = ei[:, keep], w[keep]
        key, order = torch.sort(ei[1] * n + ei[0], stable=True)            # (col, row), input order among duplicates
        w = w[order]
        uniq, inv, counts = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
        rank = torch.arange(key.numel(), device=dev) - (torch.cumsum(counts, 0) - counts)[inv]
        ws = torch.zeros(uniq.numel(), dtype=torch.float64, device=dev)
        for k in range(int(counts.max()) if counts.numel() else 0):   # duplicates summed in input order (one add per slot per pass)
            sel = rank == k
            ws.index_add_(0, inv[sel], w[sel])
        row, col = uniq % n if n else uniq, uniq // n if n else uniq
        kt, pt = torch.sort(row * n + col)
        if not (torch.equal(kt, uniq) and torch.equal(ws[pt], ws)):
            raise ValueError("adjacency not symmetric")
        present = torch.zeros(n, dtype=torch.bool, device=dev)
        present[col] = True
        iso = torch.nonzero(~present).reshape(-1)
        if iso.numel():   # (i, i, 0): the column of an id without edges
            key2, o2 = torch.sort(torch.cat([uniq, iso * n + iso]))
            row, col = torch.cat([row, iso])[o2], torch.cat([col, iso])[o2]
            ws = torch.cat([ws, torch.zeros(iso.numel(), dtype=torch.float64, device=dev)])[o2]
        sc = torch.stack([row.to(torch.float64), col.to(torch.float64), ws], 1).contiguous()
        if np_ is None:
            p = torch.tensor([0, sc.shape[0]], dtype=torch.int64)
        else:   # the rows are in column order, the graphs contiguous id ranges: graph g is the rows with node_ptr[g] <= col < node_ptr[g+1]
            p = torch.searchsorted(col.contiguous(), np_.to(dev)).to(device="cpu", dtype=torch.int64)
    return sc, p, np_, n


def ppr_diffusion(
    edge_index: Tensor,
    edge_weights: Optional[Tensor],
    num_nodes: int,
    *,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    alpha: float = 0.2,
    eps: float = 1e-4,
    tol: float = 1e-10,
    add_self_loop: bool = False,
    normalize_out: bool = True,
) -> Tuple[Tensor, Tensor]:
    """The diffusion of snapshot_ppr on a plain undirected edge list (both directions present), node set [0, num_nodes) -- what
    adapters.compute_ppr(edge_index, edge_weights, num_nodes, ...) computes densely; PyGCL's A.PPRDiffusion uses add_self_loop=True.
    Rows of weight 0 are dropped (as the op's reader does); a negative weight raises ValueError.  The rows are grouped by column with
    a stable device sort and duplicates summed (in input order); a pattern or weights that are not exactly symmetric raise
    ValueError("adjacency not symmetric").  An id without edges keeps its diagonal entry: alpha (1 with a self loop) before
    normalisation.  With `node_ptr` (G+1 offsets of a batch's contiguous id ranges) every graph is diffused on its own, as one call
    per graph would, in the one device call: the cost is the sum of n_g^2, not (sum n_g)^2; a row between two graphs raises
    ValueError.  Returns (edge_index (2, P) int64, edge_weights (P,) float64) in row-major order, on the input's device.
    """
    alpha, eps, tol, _ = _ppr_params(alpha, eps, tol)
    _num_nodes(num_nodes)
    sc, p, np_, n = _diffusion_input(edge_index, edge_weights, num_nodes, node_ptr)
    with torch.cuda.device(sc.device):
        flags = (_lib.PPR_WEIGHTED | _lib.PPR_ZERO_ROWS | (_lib.PPR_SELF_LOOP if add_self_loop else 0)
                 | (_lib.PPR_NORMALIZE if normalize_out else 0))
        out, _ = _ppr_call(sc, p, np_, n, alpha, eps, tol, flags)
        return out[:, :2].long().t().contiguous(), out[:, 2].contiguous()


MARKOV_MAX_ORDER = _lib.MARKOV_MAX_ORDER   # cap on the order D (rlap_amd/csrc/rlap_markov.h::MAX_ORDER)


def _markov_params(alpha, order, eps) -> Tuple[float, int, float]:
    """Host-side checks of the Markov diffusion's parameters, made before anything is launched."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha: a number in [0, 1], got {alpha!r}")
    if isinstance(order, bool) or not hasattr(order, "__index__") or not 1 <= order.__index__() <= MARKOV_MAX_ORDER:
        raise ValueError(f"order: an integer in [1, {MARKOV_MAX_ORDER}], got {order!r}")
    e = _real(eps, "eps", 0.0, float("inf"))
    return float(alpha), order.__index__(), e


def _markov_call(x: Tensor, p: Tensor, np_: Optional[Tensor], n: int, alpha: float, order: int, eps: float, flags: int) -> Tuple[Tensor, Tensor]:
    """One rlap_snapshot_markov call inside torch-owned memory, with _ppr_call's first output capacity and single retry."""
    global last_stats
    S, m, dev = p.numel() - 1, int(x.shape[0]), x.device
    cap = first_cap = min(S * min(n, m) ** 2, max(PPR_FIRST_CAP_PER_ROW * m + 64, PPR_FIRST_CAP_MIN))
    for retries in (0, 1):
        out = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        mptr = torch.empty(S + 1, dtype=torch.int64, device=dev)
        info = _snapshot_call("rlap_snapshot_markov", _lib.MarkovInfo, x, p, np_, n,
                              (alpha, order, eps, flags, out.data_ptr() if cap else None, cap, mptr.data_ptr()),
                              extra_msg=" (or a weight is <= 0)", accept=(_lib.E_OUT_CAPACITY,) if retries == 0 else ())
        P = int(info.rows_needed)
        if P <= cap:   # (more than the capacity: RLAP_E_OUT_CAPACITY, accepted on the first attempt only)
            break
        cap = P
    last_stats = dict(info.as_dict(), output_retries=retries, first_cap=first_cap)
    return _trim(out, P), mptr


def _markov_flags(weighted: bool, add_self_loop: bool, normalize_out: bool) -> int:
    return ((_lib.MARKOV_WEIGHTED if weighted else 0) | (_lib.MARKOV_SELF_LOOP if add_self_loop else 0)
            | (_lib.MARKOV_NORMALIZE if normalize_out else 0))


def snapshot_markov(
    sc: Tensor,
    ptr: Union[Tensor, Sequence[int]],
    num_nodes: int,
    *,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    alpha: float = 0.2,
    order: int = 16,
    eps: float = 1e-4,
    weighted: bool = True,
    add_self_loop: bool = True,
    normalize_out: bool = False,
) -> Tuple[Tensor, Tensor]:
    """Markov diffusion of every snapshot of a result of the calls above, on the device and without a dense matrix.  `sc`, `ptr`,
    `num_nodes` and `node_ptr` as for snapshot_stats.  This restates the published `GCL.augmentors.functional.
    compute_markov_diffusion` (PyGCL is not installed here: the definition is unpinned, not a run of that function; it calls
    `order` `degree`).

    For snapshot s with distinct ids V_s and symmetric adjacency A (the rows' weights, or unit entries with weighted=False; duplicate
    rows summed; A + I with add_self_loop), d = A 1, Â = D^-1/2 A D^-1/2 (0 where d = 0), beta = 1 - alpha, D = order:
        z = Â; t = Â; D times: t = beta Â t, z += t; z /= D; z += alpha Â
        M = alpha Â + (1/D) sum_{k=0..D} beta^k Â^(k+1),  entries M_ij >= eps kept,  normalize_out: D_M^-1/2 M D_M^-1/2 (row sums)
    Returns (out (P, 3) float64 rows [i, j, value] in the input's id space, mptr (S+1,) int64), both on sc's device: segment s is rows
    [mptr[s], mptr[s+1]) in row-major order (ascending i, then j), the layout of snapshot_ppr.  Every column is computed in Horner
    form by D + 1 applications of Â (rlap_amd/csrc/rlap_markov.h holds every scalar step, so a g++ build of that header computes
    the same bits).  The result is exactly symmetric, the same input gives the same bits, and segment s equals the same call on that
    segment alone, bit for bit.  An id without edges keeps no row without the self loop and the one entry alpha + (1/D) sum_k beta^k
    with it.

    alpha outside [0, 1], order outside [1, MARKOV_MAX_ORDER], eps <= 0, malformed tables, a column not contiguous within its
    segment, a row id without a column, an id out of range, or (weighted) a weight <= 0 raise ValueError.  `last_stats` then holds
    what the call did (rlap_markov_info: order, small / large tiles, groups, launches, rows_needed, arena_bytes, host_syncs)
    and `output_retries` (1 when the first capacity guess was short).
    """
    p, np_ = _snapshot_tables(sc, ptr, num_nodes, node_ptr)
    alpha, order, eps = _markov_params(alpha, order, eps)
    if weighted and not sc.is_cuda and sc.shape[0] and not bool((sc[:, 2] > 0).all() and torch.isfinite(sc[:, 2]).all()):
        raise ValueError("sc: every weight must be > 0")
    dev = _device_for(sc)
    flags = _markov_flags(weighted, add_self_loop, normalize_out)
    with torch.cuda.device(dev):
        x = sc.to(device=dev, dtype=torch.float64).contiguous()
        return _markov_call(x, p, np_, int(num_nodes), alpha, order, eps, flags)


def markov_diffusion(
    edge_index: Tensor,
    edge_weights: Optional[Tensor],
    num_nodes: int,
    *,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    alpha: float = 0.2,
    order: int = 16,
    eps: float = 1e-4,
    add_self_loop: bool = True,
    normalize_out: bool = False,
) -> Tuple[Tensor, Tensor]:
    """The diffusion of snapshot_markov on a plain undirected edge list (both directions present), node set [0, num_nodes) -- what
    adapters.compute_markov_diffusion(edge_index, edge_weights, num_nodes, ...) computes densely.  The list is prepared as for
    ppr_diffusion (rows of weight 0 dropped, grouped by column, duplicates summed in input order, symmetry checked, ids without
    edges kept as (i, i, 0)).  With `node_ptr` (G+1 offsets of a batch's contiguous id ranges) every graph is a segment of its own:
    a batch costs the sum of n_g^2, not (sum n_g)^2; a row between two graphs raises
    ValueError.  Returns (edge_index (2, P) int64, edge_weights (P,) float64) in row-major order, on the input's device.
    """
    alpha, order, eps = _markov_params(alpha, order, eps)
    _num_nodes(num_nodes)
    sc, p, np_, n = _diffusion_input(edge_index, edge_weights, num_nodes, node_ptr)
    with torch.cuda.device(sc.device):
        out, _ = _markov_call(sc, p, np_, n, alpha, order, eps, _markov_flags(True, add_self_loop, normalize_out) | _lib.MARKOV_ZERO_ROWS)
        return out[:, :2].long().t().contiguous(), out[:, 2].contiguous()


def _subgraph_args(sc: Tensor, ptr, num_nodes: int, nodes, nodes_ptr, node_ptr):
    """Host-side checks of snapshot_subgraph, made before anything is launched: (ptr, node_ptr, nodes, nodes_ptr), the tables as
    int64 CPU tensors, `nodes` as given (a tensor, on its device) or made from a sequence."""
    try:
        single = len(ptr) == 1
    except TypeError:
        single = False
    if single:
        # S = 0: no segment at all (ptr == [0], no rows); sc, num_nodes and node_ptr keep their rules
        rows = int(sc.shape[0]) if isinstance(sc, Tensor) and sc.dim() == 2 else 0
        _snapshot_tables(sc, [0, rows], num_nodes, None)
        p = _int_tensor(ptr, "ptr").reshape(-1).contiguous()
        if p.numel() != 1 or int(p[0]) != 0 or rows != 0:
            raise ValueError("ptr: a single offset describes no segment and needs ptr == [0] and no rows")
        np_ = _ptr_table(node_ptr, "node_ptr", 0, num_nodes.__index__()) if node_ptr is not None else None
    else:
        p, np_ = _snapshot_tables(sc, ptr, num_nodes, node_ptr)
    S = p.numel() - 1
    if nodes is None:
        if nodes_ptr is not None:
            raise ValueError("nodes_ptr: only together with nodes")
        return p, np_, None, None
    if isinstance(nodes, Tensor):
        if nodes.dtype.is_floating_point or nodes.dtype.is_complex or nodes.dtype == torch.bool:
            raise ValueError("nodes: integers only")
        nd = nodes.detach()
    else:
        nd = _int_tensor(nodes, "nodes")
    if nd.dim() != 1:
        raise ValueError("nodes: a 1-D tensor of node ids")
    q = None
    if nodes_ptr is not None:
        q = _ptr_table(nodes_ptr, "nodes_ptr", 0, int(nd.numel())) if S > 0 else _int_tensor(nodes_ptr, "nodes_ptr")
        if q.dim() != 1 or q.numel() != S + 1:
            raise ValueError(f"nodes_ptr: {S + 1} offsets (one list per segment), got {tuple(q.shape)}")
        if S == 0 and (int(q[0]) != 0 or nd.numel() != 0):
            raise ValueError("nodes_ptr: non-decreasing offsets from 0 to len(nodes)")
    return p, np_, nd, q


def snapshot_subgraph(
    sc: Tensor,
    ptr: Union[Tensor, Sequence[int]],
    num_nodes: int,
    nodes: Optional[Union[Tensor, Sequence[int]]] = None,
    nodes_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    relabel: bool = False,
    remove_self_loops: bool = False,
) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The induced subgraph of every snapshot on a node set, optionally with compact ids -- the torch.unique + subgraph(...,
    relabel_nodes=True) step of the reference's scripts (scripts/rlap_vc_spectral.py:42-51, scripts/augmentor_benchmarks.py:121-171,
    scripts/rlap_ppr_edge_plots.py:61-76) for all snapshots of one call, on the device and without a sort.  `sc`, `ptr`, `num_nodes`
    and `node_ptr` as for snapshot_stats, but the rows of a segment may come in any order and need not be symmetric: the result of
    every elimination entry point, of snapshot_ppr, or a plain edge list.  ptr == [0] (no segment) is allowed.

    Node sets: `nodes=None` takes the ids that appear in the segment's rows (torch.unique of the snapshot).  `nodes` with
    `nodes_ptr` (S+1 offsets) is one list per segment, `nodes` alone one list for all segments (with `node_ptr` a segment takes the
    part of the list inside its graph's range).  Lists are sets: any order, repeats allowed, and an id that no row has still takes a
    label.  `remove_self_loops` drops the rows with i == j, and with nodes=None they do not put i into the set (remove_self_loops
    before unique).  `relabel` replaces the ids of the kept rows by their rank among the sorted ids of the set, from 0 in every
    segment -- PyG's relabel_nodes=True for a sorted, distinct subset such as a torch.unique result.

    Returns (out, optr, ids, iptr) on sc's device: out[optr[s]:optr[s+1]] the kept rows of segment s in their input order, the weight
    column copied bit for bit; ids[iptr[s]:iptr[s+1]] its node set, sorted -- the map label -> id.  The same input gives the same
    bits.  Malformed tables, or an id of a row or list outside its segment's range, raise ValueError.  `last_stats` then holds what the
    call did (rlap_subgraph_info: rows_kept, ids_written, arena_bytes, host_syncs).
    """
    p, np_, nd, q = _subgraph_args(sc, ptr, num_nodes, nodes, nodes_ptr, node_ptr)
    S, G, n = p.numel() - 1, _graphs(np_), int(num_nodes)
    dev = _device_for(sc)
    flags = (_lib.SUB_RELABEL if relabel else 0) | (_lib.SUB_NO_SELF_LOOPS if remove_self_loops else 0)
    with torch.cuda.device(dev):
        x = sc.to(device=dev, dtype=torch.float64).contiguous()
        m = int(x.shape[0])
        d_nd = nd.to(device=dev, dtype=torch.int64).contiguous() if nd is not None else None
        d_q = q.to(dev) if q is not None else None
        L = len(d_nd) if d_nd is not None else 0
        cap = min(2 * m, (S // G) * n) if d_nd is None else (L if d_q is not None else (S // G) * L)
        out = torch.empty((m, 3), dtype=torch.float64, device=dev)
        optr = torch.empty(S + 1, dtype=torch.int64, device=dev)
        ids = torch.empty(cap, dtype=torch.int64, device=dev)
        iptr = torch.empty(S + 1, dtype=torch.int64, device=dev)
        info = _snapshot_call("rlap_snapshot_subgraph", _lib.SubgraphInfo, x, p, np_, n, (
            (d_nd.data_ptr() or iptr.data_ptr()) if d_nd is not None else None,   # (an empty list is still a list: not NULL)
            d_q.data_ptr() if d_q is not None else None, L,
            flags, out.data_ptr() if m else None, optr.data_ptr(), ids.data_ptr() if cap else None, cap, iptr.data_ptr()), grouped=False)
        return _trim(out, int(info.rows_kept)), optr, _trim(ids, int(info.ids_written)), iptr


def snapshot_gcn_norm(
    sc: Tensor,
    ptr: Union[Tensor, Sequence[int]],
    num_nodes: int,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    weighted: bool = False,
    add_self_loops: bool = True,
    fill_value: float = 1.0,
    normalize: bool = True,
    dtype: torch.dtype = torch.float32,
) -> Tuple[Tensor, Tensor, Tensor]:
    """Every snapshot of a call as the encoder eats it: the int64 `edge_index`, the self loops and the symmetric normalisation
    coefficients -- sc[:, :2].long().t().contiguous() followed by what GCNConv does first with every view (PyG's gcn_norm:
    add_remaining_self_loops, the degree scatter, deg^-1/2, one product per edge; scripts/node_shared.py:242-245), for all
    snapshots at once, in one pass over the rows and without float atomics.  `sc`, `ptr`, `num_nodes` and `node_ptr` as for
    snapshot_stats, in the same layout (rows of a segment grouped by column id, every row id with a column block of its own: the
    result of every elimination entry point).  The (out, pptr) of snapshot_ppr (grouped by row id) and arbitrary edge lists are not
    in that layout and are refused or out of scope.  `num_nodes` may exceed the elimination's (eliminated and isolated ids get a loop).

    Row id = source, column id = target, as gcn_norm(flow="source_to_target") reads edge_index = sc[:, :2].long().t().  (Unpinned: PyG
    is not installed here; this follows its published semantics, not a run of it.)  Per segment s with id range [lo, hi):
      weighted        : the rows' weights, else every row weighs 1 (the reference's rLap returns edge_weights=None)
      add_self_loops  : rows with row == col leave the list, the others keep their input order, then one loop (i, i) for every i in
                        [lo, hi) ascending; it weighs `fill_value` (2.0 is PyG's improved=True) unless the segment had loop rows of i:
                        then the last one's weight (1 when unweighted).  False: the rows as they are
      normalize       : value (i, j, w) = dis[i] * w * dis[j], dis = deg^-1/2 (0 where deg == 0), deg[j] the sum of the weights of the
                        entries whose target is j.  False: w itself -- the call is then the conversion alone, plus loops if asked
      dtype           : torch.float32 (the float64 value rounded once) or torch.float64

    Returns (edge_index, weight, eptr) on sc's device: ONE contiguous (2, M) int64 tensor, the (M,) values and the S+1 entry offsets;
    snapshot s is edge_index[:, eptr[s]:eptr[s+1]], weight[eptr[s]:eptr[s+1]] -- feed it to GCNConv(..., normalize=False).  The same
    input gives the same bits, and a segment's values do not depend on the other segments of the call.  Malformed tables, a layout
    error, or (weighted and normalize) a weight that is not finite or <= 0 raise ValueError.  `last_stats` then holds what the call did
    (rlap_gcn_info: entries, loops_removed, arena_bytes, host_syncs).
    """
    p, np_ = _snapshot_tables(sc, ptr, num_nodes, node_ptr)
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"dtype: torch.float32 or torch.float64, got {dtype!r}")
    fill = _real(fill_value, "fill_value", 0.0, float("inf"))
    S, G, n = p.numel() - 1, _graphs(np_), int(num_nodes)
    dev = _device_for(sc)
    flags = ((_lib.GCN_WEIGHTED if weighted else 0) | (_lib.GCN_SELF_LOOPS if add_self_loops else 0)
             | (_lib.GCN_NORMALIZE if normalize else 0) | (_lib.GCN_F32 if dtype == torch.float32 else 0))
    with torch.cuda.device(dev):
        x = sc.to(device=dev, dtype=torch.float64).contiguous()
        cap = int(x.shape[0]) + ((S // G) * n if add_self_loops else 0)
        ei = torch.empty((2, cap), dtype=torch.int64, device=dev)
        val = torch.empty(cap, dtype=dtype, device=dev)
        eptr = torch.empty(S + 1, dtype=torch.int64, device=dev)
        info = _snapshot_call("rlap_snapshot_gcn_norm", _lib.GcnInfo, x, p, np_, n, (
            flags, fill, ei[0].data_ptr() if cap else None, ei[1].data_ptr() if cap else None, val.data_ptr() if cap else None, cap,
            eptr.data_ptr()))
        M = int(info.entries)
        if M != cap:   # (only an input with loop rows: the two rows of edge_index move together)
            ei, val = ei[:, :M].contiguous(), val[:M].clone()
        return ei, val, eptr


def _features_arg(x, n: int, L: int) -> bool:
    """The checks of the features of a propagation, (n, F) or (L, n, F): whether there is one matrix per layer."""
    if not isinstance(x, Tensor) or x.dim() not in (2, 3):
        raise ValueError("x: a (num_nodes, F) or (layers, num_nodes, F) tensor")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"x: torch.float32 or torch.float64, got {x.dtype}")
    if x.shape[-2] != n:
        raise ValueError(f"x: {x.shape[-2]} rows, num_nodes is {n}")
    if x.dim() == 3 and x.shape[0] != L:
        raise ValueError(f"x: {x.shape[0]} layers, the call has {L} (segments / graphs)")
    if x.shape[-1] < 1:
        raise ValueError("x: at least one feature column")
    return x.dim() == 3


def _propagate_args(sc, ptr, num_nodes, x, node_ptr, fill_value):
    """Host-side checks of snapshot_propagate, made before the device is touched: (ptr, node_ptr, fill, layers, per_layer)."""
    p, np_ = _snapshot_tables(sc, ptr, num_nodes, node_ptr)
    fill = _real(fill_value, "fill_value", 0.0, float("inf"))
    S, G = p.numel() - 1, _graphs(np_)
    if S < 1 or S % G != 0:
        raise ValueError(f"ptr: {S} segments; at least one, and a multiple of the {G} graphs")
    L = S // G
    return p, np_, fill, L, _features_arg(x, int(num_nodes), L)


def _propagate(sc, p, np_, n, x, L, per_layer, weighted, add_self_loops, fill, normalize, transpose):
    """One rlap_snapshot_propagate call; x is already checked."""
    dev = _device_for(sc)
    flags = ((_lib.GCN_WEIGHTED if weighted else 0) | (_lib.GCN_SELF_LOOPS if add_self_loops else 0)
             | (_lib.GCN_NORMALIZE if normalize else 0) | (_lib.SPMM_TRANSPOSE if transpose else 0)
             | (_lib.SPMM_X_F32 if x.dtype == torch.float32 else 0) | (_lib.SPMM_X_PER_LAYER if per_layer else 0))
    with torch.cuda.device(dev):
        rows = sc.to(device=dev, dtype=torch.float64).contiguous()
        d_x = x.detach().to(device=dev).contiguous()
        F = int(d_x.shape[-1])
        y = torch.empty((L, n, F), dtype=d_x.dtype, device=dev)
        _snapshot_call("rlap_snapshot_propagate", _lib.SpmmInfo, rows, p, np_, n,
                       (flags, fill, d_x.data_ptr() if d_x.numel() else None, F, y.data_ptr() if y.numel() else None))
        return y


class _Propagate(torch.autograd.Function):
    """y = A^ x; the gradient with respect to x is the transposed product of the gradient of y (summed over the layers when one x
    serves them all).  sc is a sample and gets none."""

    @staticmethod
    def forward(ctx, x, call):
        ctx.call = call
        return _propagate(*call[:4], x, *call[4:])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        sc, p, np_, n, L, per_layer, weighted, loops, fill, normalize, transpose = ctx.call
        gx = _propagate(sc, p, np_, n, gy.contiguous(), L, True, weighted, loops, fill, normalize, not transpose)
        return (gx if per_layer else gx.sum(0)), None


def snapshot_propagate(
    sc: Tensor,
    ptr: Union[Tensor, Sequence[int]],
    num_nodes: int,
    x: Tensor,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    weighted: bool = False,
    add_self_loops: bool = True,
    fill_value: float = 1.0,
    normalize: bool = True,
    transpose: bool = False,
) -> Tensor:
    """The sparse product of a GCN layer for every snapshot of a call at once: y[l] = A^_l x, with A^_l the list that
    snapshot_gcn_norm(sc, ptr, num_nodes, node_ptr, weighted, add_self_loops, fill_value, normalize) produces for layer l -- what
    GCNConv(..., normalize=False) does next with that list (scripts/node_shared.py: two views, three encodes a step) -- without the
    list, without float atomics and in a fixed order.  `sc`, `ptr`, `num_nodes`, `node_ptr` and the four list arguments as for
    snapshot_gcn_norm.  The S segments are L = S / G layers (view x depth) of G graphs each; the graphs of a layer cover disjoint ids.

      x         : (num_nodes, F), one feature matrix for all layers (the first GCN layer of every view), or (L, num_nodes, F), one
                  per layer (the later ones); float32 or float64, on any device (moved to sc's)
      transpose : the transposed product, y[l, i] = the sum over the entries with SOURCE i of c_e x[target] (the backward pass; with
                  o_v="random" the two weights of a pair may differ in the last bit, so A^ is symmetric only up to that)
    Returns y, (L, num_nodes, F) of x's dtype on sc's device: y[l, j] = the sum over the entries e with target j of c_e x[source(e)],
    c_e the float64 coefficient of snapshot_gcn_norm (the same bits), summed in float64 in list order -- the rows of j's block in
    input order, then the loop; lists longer than 256 entries in chunks of 256 (rlap_amd/csrc/rlap_spmm.h) -- and rounded once for
    float32.  The same input gives the same bits; a segment's result does not depend on the others.  An id without rows and
    without a loop gets 0.

    Differentiable in x (its backward is the same call with `transpose` flipped); `sc` gets no gradient, and double backward is not
    supported.  Malformed arguments raise ValueError before the device is touched; layout errors raise ValueError as for
    snapshot_gcn_norm.  `last_stats` then holds what the call did (rlap_spmm_info: entries, blocks, chunked_lists, arena_bytes,
    host_syncs).
    """
    p, np_, fill, L, per_layer = _propagate_args(sc, ptr, num_nodes, x, node_ptr, fill_value)
    call = (sc, p, np_, int(num_nodes), L, per_layer, bool(weighted), bool(add_self_loops), fill, bool(normalize), bool(transpose))
    if torch.is_grad_enabled() and x.requires_grad:
        return _Propagate.apply(x, call)
    return _propagate(sc, p, np_, int(num_nodes), x, L, per_layer, *call[6:])


READOUT_REDUCE = {"sum": 0, "mean": _lib.READOUT_MEAN}


class GraphTable:
    """The `node_ptr` of a batch as graph_readout takes it, checked once: `host` the int64 CPU table (non-decreasing from 0 to
    `num_nodes`), `graphs` its G, `chunks` and `chunked_graphs` what rlap_readout_info reports as bounds, counted exactly here
    (rlap_amd/csrc/rlap_readout.h: chunks of 256 ids, graphs of more than one chunk).  `on(device)` is the device copy, made once
    per device and kept.  A holder that reads out after every layer (adapters.Snapshots.readout) keeps one of these."""

    def __init__(self, node_ptr, num_nodes: int):
        self.num_nodes = _num_nodes(num_nodes)
        self.host = _ptr_table(node_ptr, "node_ptr", 0, self.num_nodes)
        self.graphs = self.host.numel() - 1
        counts = self.host[1:] - self.host[:-1]
        self.chunks = int(((counts + 255) // 256).sum())
        self.chunked_graphs = int((counts > 256).sum())
        self._dev = {}

    def on(self, device) -> Tensor:
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.host.to(device)
        return self._dev[key]


def _graph_table(node_ptr, n: int) -> GraphTable:
    """The GraphTable of a call on n nodes: the caller's own, checked against n, or one made from its node_ptr."""
    if not isinstance(node_ptr, GraphTable):
        return GraphTable(node_ptr, n)
    if node_ptr.num_nodes != n:
        raise ValueError(f"node_ptr[-1] ({node_ptr.num_nodes}) must equal {n}")
    return node_ptr


def _readout_args(x, node_ptr, reduce):
    """Host-side checks of graph_readout, made before the device is touched: (table, flags without the type)."""
    if not isinstance(x, Tensor) or x.dim() not in (2, 3):
        raise ValueError("x: a (num_nodes, F) or (layers, num_nodes, F) tensor")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"x: torch.float32 or torch.float64, got {x.dtype}")
    if x.shape[-1] < 1:
        raise ValueError("x: at least one feature column")
    if not isinstance(reduce, str) or reduce not in READOUT_REDUCE:
        raise ValueError(f"reduce: one of {sorted(READOUT_REDUCE)}, got {reduce!r}")
    return _graph_table(node_ptr, int(x.shape[-2])), READOUT_REDUCE[reduce]


def _readout(export: str, x: Tensor, table: GraphTable, flags: int, rows_out: int) -> Tensor:
    """One rlap_graph_readout / _backward call: x is (L, rows, F) and checked, the result (L, rows_out, F) on the library's device."""
    dev = _device_for(x)
    flags |= _lib.READOUT_X_F32 if x.dtype == torch.float32 else 0
    with torch.cuda.device(dev):
        d_x = x.detach().to(device=dev).contiguous()
        L, F, N, G = int(d_x.shape[0]), int(d_x.shape[2]), table.num_nodes, table.graphs
        out = torch.empty((L, rows_out, F), dtype=d_x.dtype, device=dev)
        _device_call(export, _lib.ReadoutInfo, dev, G, (
            d_x.data_ptr() if d_x.numel() else None, L, N, F, table.on(dev).data_ptr(), G, flags, out.data_ptr() if out.numel() else None))
    last_stats.update(chunks=table.chunks, chunked_graphs=table.chunked_graphs)   # (exact: this host has read the table)
    return out


class _Readout(torch.autograd.Function):
    """y = the per-graph sum (mean) of x; the gradient with respect to x is the gather of the backward export."""

    @staticmethod
    def forward(ctx, x, table, flags):
        ctx.call = (table, flags)
        return _readout("rlap_graph_readout", x, table, flags, table.graphs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        table, flags = ctx.call
        return _readout("rlap_graph_readout_backward", gy.contiguous(), table, flags, table.num_nodes), None, None


def graph_readout(x: Tensor, node_ptr: Union[Tensor, Sequence[int], GraphTable], reduce: str = "sum") -> Tensor:
    """The readout of a batch of graphs: y[g] = the sum (reduce="mean": the mean) of the rows x[i] of graph g's nodes,
    node_ptr[g] <= i < node_ptr[g+1] -- global_add_pool(z, batch) of the graph-level training step (scripts/graph_shared.py: after
    every GIN layer), without float atomics and in a fixed order.

      x        : (num_nodes, F), returning (G, F), or (L, num_nodes, F) -- the embeddings of L views at once -- returning (L, G, F);
                 float32 or float64, on any device (moved to the library's)
      node_ptr : [G+1] offsets, non-decreasing from 0 to num_nodes (adapters.node_ptr_of turns a PyG `batch` vector into one),
                 checked on the host; or a GraphTable, which keeps the check and the device copy for the next call
      reduce   : "sum" or "mean"
    One element is the rule of rlap_amd/csrc/rlap_spmm.h on the graph's rows in id order: float64 terms, chunks of 256 rows summed
    from 0, the chunk sums added in chunk order; the mean divides that sum once, in float64, by the number of nodes; an empty graph
    gives exactly 0; a float32 result is the float64 value rounded once.  The same input gives the same bits, and a graph's result
    does not depend on the other graphs, on L or on F.

    Differentiable in x (the backward is one gather, rlap_graph_readout_backward); double backward is not supported.  Malformed
    arguments raise ValueError before the device is touched.  No host synchronisation.  `last_stats` then holds what the call did
    (rlap_readout_info: rows, graphs, chunks, chunked_graphs -- counted exactly from the host's table --, arena_bytes, host_syncs).
    """
    table, flags = _readout_args(x, node_ptr, reduce)
    x3 = x if x.dim() == 3 else x.unsqueeze(0)
    if torch.is_grad_enabled() and x.requires_grad:
        y = _Readout.apply(x3, table, flags)
    else:
        y = _readout("rlap_graph_readout", x3, table, flags, table.graphs)
    return y if x.dim() == 3 else y[0]


INFONCE_POSITIVE = {"scaled": 0, "raw": _lib.INFONCE_POSITIVE_RAW}
INFONCE_MAX_F = 512
INFONCE_TAU = (1.0 / 32.0, 1024.0)
INFONCE_INTRAVIEW = {"none": 0, "masked": _lib.INFONCE_INTRA_MASKED, "all": _lib.INFONCE_INTRA_ALL}


def _info_nce_args(anchor, sample, tau, positive):
    """Host-side checks of info_nce, made before the device is touched: (tau, flags)."""
    for t, what in ((anchor, "anchor"), (sample, "sample")):
        if not isinstance(t, Tensor) or t.dim() != 2:
            raise ValueError(f"{what}: a (num_nodes, F) tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: torch.float32, got {t.dtype}")
    if anchor.shape != sample.shape:
        raise ValueError(f"anchor and sample: equal shapes, got {tuple(anchor.shape)} and {tuple(sample.shape)}")
    n, f = int(anchor.shape[0]), int(anchor.shape[1])
    if n < 1 or f < 1:
        raise ValueError("anchor: at least one row and one feature column")
    if f > INFONCE_MAX_F:
        raise ValueError(f"anchor: at most {INFONCE_MAX_F} feature columns, got {f}")
    if n >= 1 << 31:
        raise ValueError("anchor: fewer than 2^31 rows")
    if isinstance(tau, bool) or not isinstance(tau, (int, float)):
        raise ValueError(f"tau: a number, got {tau!r}")
    tau = float(tau)
    if not INFONCE_TAU[0] <= tau <= INFONCE_TAU[1]:
        raise ValueError(f"tau: must lie in [{INFONCE_TAU[0]}, {INFONCE_TAU[1]}], got {tau!r}")
    if not isinstance(positive, str) or positive not in INFONCE_POSITIVE:
        raise ValueError(f"positive: one of {sorted(INFONCE_POSITIVE)}, got {positive!r}")
    return tau, INFONCE_POSITIVE[positive]


def _info_nce_intraview(intraview):
    """The `intraview` keyword of info_nce and info_nce_pair as the C ABI's value; 0 is "none", which takes the plain exports."""
    if not isinstance(intraview, str) or intraview not in INFONCE_INTRAVIEW:
        raise ValueError(f"intraview: one of {sorted(INFONCE_INTRAVIEW)}, got {intraview!r}")
    return INFONCE_INTRAVIEW[intraview]


def _intra_call(name, intra, args):
    """(export, arguments) of an InfoNCE call: the plain export with today's arguments, or its _intra twin with the variant behind
    `flags` (the sixth argument after the handle)."""
    if not intra:
        return name, args
    stem, back = (name[:-len("_backward")], "_backward") if name.endswith("_backward") else (name, "")
    return stem + "_intra" + back, args[:6] + (intra,) + args[6:]


def _info_nce_forward(a: Tensor, b: Tensor, tau: float, flags: int, intra: int = 0):
    """The forward export: (loss 0-dim, rows [N], z [N], the device copies of a and b)."""
    dev = _device_for(a)
    with torch.cuda.device(dev):
        d_a = a.detach().to(device=dev).contiguous()
        d_b = b.detach().to(device=dev).contiguous()
        n, f = int(d_a.shape[0]), int(d_a.shape[1])
        out = torch.empty(1 + 2 * n, dtype=torch.float64, device=dev)   # loss | rows | z
        p = out.data_ptr()
        export, args = _intra_call("rlap_infonce", intra, (d_a.data_ptr(), d_b.data_ptr(), n, f, tau, flags, p, p + 8, p + 8 * (1 + n)))
        _device_call(export, _lib.InfonceInfo, dev, 1, args)
    return out[0], out[1:1 + n], out[1 + n:], d_a, d_b


class _InfoNCE(torch.autograd.Function):
    """loss = the fused InfoNCE of (anchor, sample); the gradients with respect to both come from the backward export."""

    @staticmethod
    def forward(ctx, a, b, tau, flags, intra):
        loss, rows, z, d_a, d_b = _info_nce_forward(a, b, tau, flags, intra)
        ctx.save_for_backward(d_a, d_b, z)
        ctx.call = (tau, flags, intra, a.device, b.device)
        ctx.mark_non_differentiable(rows)
        return loss, rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_rows):
        d_a, d_b, z = ctx.saved_tensors
        tau, flags, intra, dev_a, dev_b = ctx.call
        dev = d_a.device
        with torch.cuda.device(dev):
            d_g = _upstream(g, dev)
            n, f = int(d_a.shape[0]), int(d_a.shape[1])
            ga = torch.empty_like(d_a)
            gb = torch.empty_like(d_b)
            export, args = _intra_call("rlap_infonce_backward", intra, (
                d_a.data_ptr(), d_b.data_ptr(), n, f, tau, flags, z.data_ptr(), d_g.data_ptr(), ga.data_ptr(), gb.data_ptr()))
            _device_call(export, _lib.InfonceInfo, dev, 1, args)
        return ga.to(dev_a), gb.to(dev_b), None, None, None


def info_nce(anchor: Tensor, sample: Tensor, tau: float = 0.4, positive: str = "scaled", return_rows: bool = False, intraview: str = "none"):
    """The InfoNCE contrastive loss of two views' node embeddings, fused on the device (rlap_infonce): with the rows
    normalised, s = ah bh^T, loss = -mean_i(c s_ii - log sum_j exp(s_ij / tau)) -- one direction of
    DualBranchContrast(InfoNCEBatched(tau), mode="L2L") (scripts/node_shared.py) without the N x N similarity matrix.

      anchor, sample : (N, F) float32 of equal shape, F <= 512, on any device (moved to the library's)
      tau            : the temperature, in [1/32, 1024]
      positive       : "scaled" -- c = 1 / tau, GCL's InfoNCE; "raw" -- c = 1, the reference's InfoNCEBatched, which does not
                       divide the positive term by tau
      return_rows    : also return the (N,) float64 row terms c s_ii - 1/tau - log Z_i (not differentiable)
      intraview      : intraview negatives, the sampler's intraview_negs=True (rlap_infonce_intra): "none" -- the
                       denominator holds the sample's rows alone; "masked" -- and the anchor's other rows j != i (GCL's InfoNCE
                       under the sampler's masks: the loss GRACE was published with); "all" -- and every anchor row, row i itself
                       included (the reference's InfoNCEBatched under the same sampler, which never reads the masks)
    Returns the 0-dim float64 loss.  The positive of row i is column i; every column is in the denominator.  Every value and the
    order of every sum are fixed (rlap_amd/csrc/rlap_infonce.h): the same input gives the same bits.  Memory is O(N F).

    Differentiable in both inputs (the backward recomputes the similarities, rlap_infonce_backward); double backward is not
    supported.  Malformed arguments raise ValueError before the device is touched; features that are not finite give a NaN loss.
    No host synchronisation.  `last_stats` then holds what the call did (rlap_infonce_info: rows, features, parts, arena_bytes,
    host_syncs).
    """
    tau, flags = _info_nce_args(anchor, sample, tau, positive)
    intra = _info_nce_intraview(intraview)
    if torch.is_grad_enabled() and (anchor.requires_grad or sample.requires_grad):
        loss, rows = _InfoNCE.apply(anchor, sample, tau, flags, intra)
    else:
        loss, rows = _info_nce_forward(anchor, sample, tau, flags, intra)[:2]
    return (loss, rows) if return_rows else loss


def _info_nce_pair_forward(a: Tensor, b: Tensor, tau: float, flags: int, intra: int = 0):
    """The pair's forward export: (loss 0-dim, rows [2, N], z [2, N], the device copies of a and b)."""
    dev = _device_for(a)
    with torch.cuda.device(dev):
        d_a = a.detach().to(device=dev).contiguous()
        d_b = b.detach().to(device=dev).contiguous()
        n, f = int(d_a.shape[0]), int(d_a.shape[1])
        out = torch.empty(1 + 4 * n, dtype=torch.float64, device=dev)   # loss | rows (2N) | z (2N)
        p = out.data_ptr()
        export, args = _intra_call("rlap_infonce_pair", intra, (d_a.data_ptr(), d_b.data_ptr(), n, f, tau, flags, p, p + 8, p + 8 * (1 + 2 * n)))
        _device_call(export, _lib.InfoncePairInfo, dev, 1, args)
    return out[0], out[1:1 + 2 * n].view(2, n), out[1 + 2 * n:].view(2, n), d_a, d_b


class _InfoNCEPair(torch.autograd.Function):
    """loss = the symmetric InfoNCE of two views; the gradients with respect to both come from one call of the backward export."""

    @staticmethod
    def forward(ctx, a, b, tau, flags, intra):
        loss, rows, z, d_a, d_b = _info_nce_pair_forward(a, b, tau, flags, intra)
        ctx.save_for_backward(d_a, d_b, z)
        ctx.call = (tau, flags, intra, a.device, b.device)
        ctx.mark_non_differentiable(rows)
        return loss, rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_rows):
        d_a, d_b, z = ctx.saved_tensors
        tau, flags, intra, dev_a, dev_b = ctx.call
        dev = d_a.device
        with torch.cuda.device(dev):
            d_g = _upstream(g, dev)
            n, f = int(d_a.shape[0]), int(d_a.shape[1])
            ga = torch.empty_like(d_a)
            gb = torch.empty_like(d_b)
            export, args = _intra_call("rlap_infonce_pair_backward", intra, (
                d_a.data_ptr(), d_b.data_ptr(), n, f, tau, flags, z.data_ptr(), d_g.data_ptr(), ga.data_ptr(), gb.data_ptr()))
            _device_call(export, _lib.InfoncePairInfo, dev, 1, args)
        return ga.to(dev_a), gb.to(dev_b), None, None, None


def info_nce_pair(h1: Tensor, h2: Tensor, tau: float = 0.4, positive: str = "scaled", return_rows: bool = False, intraview: str = "none"):
    """The symmetric InfoNCE loss of two views, 0.5 * (info_nce(h1, h2) + info_nce(h2, h1)), from one pass over the similarities
    (rlap_infonce_pair): what DualBranchContrast(InfoNCEBatched(tau), mode="L2L") computes for both directions.  The
    similarity of the second direction is the transpose of the first's bit for bit, so the row sums and the column sums of one set
    of tiles are the two denominators, and the backward folds both directions into one weight: five N x N x F products a step where
    the two info_nce calls make ten.

      h1, h2, tau, positive : as info_nce
      return_rows           : also return the (2, N) float64 row terms: those of (h1, h2), then those of (h2, h1) (not differentiable)
      intraview             : as info_nce: each direction's denominator also holds its anchor view's own rows
                              (rlap_infonce_pair_intra)
    Returns the 0-dim float64 loss; it equals the two-call value up to the order of the sums, which is fixed here too
    (rlap_amd/csrc/rlap_infonce.h): the same input gives the same bits.  Memory is O(N F).

    Differentiable in both inputs (one rlap_infonce_pair_backward call); double backward is not supported.  Malformed arguments
    raise ValueError before the device is touched.  No host synchronisation.  `last_stats` then holds what the call did
    (rlap_infonce_pair_info: rows, features, arena_bytes, parts, groups, host_syncs).
    """
    tau, flags = _info_nce_args(h1, h2, tau, positive)
    intra = _info_nce_intraview(intraview)
    if torch.is_grad_enabled() and (h1.requires_grad or h2.requires_grad):
        loss, rows = _InfoNCEPair.apply(h1, h2, tau, flags, intra)
    else:
        loss, rows = _info_nce_pair_forward(h1, h2, tau, flags, intra)[:2]
    return (loss, rows) if return_rows else loss


CCA_MAX_F = 512


def _cca_args(h1, h2, lambd):
    """Host-side checks of cca_loss, made before the device is touched: lambd as a float."""
    for t, what in ((h1, "h1"), (h2, "h2")):
        if not isinstance(t, Tensor) or t.dim() != 2:
            raise ValueError(f"{what}: a (num_nodes, F) tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: torch.float32, got {t.dtype}")
    if h1.shape != h2.shape:
        raise ValueError(f"h1 and h2: equal shapes, got {tuple(h1.shape)} and {tuple(h2.shape)}")
    if h1.device != h2.device:
        raise ValueError(f"h1 and h2: one device, got {h1.device} and {h2.device}")
    n, f = int(h1.shape[0]), int(h1.shape[1])
    if n < 2:
        raise ValueError("h1: at least two rows (the unbiased deviation divides by N - 1)")
    if f < 1:
        raise ValueError("h1: at least one feature column")
    if f > CCA_MAX_F:
        raise ValueError(f"h1: at most {CCA_MAX_F} feature columns, got {f}")
    if n >= 1 << 31:
        raise ValueError("h1: fewer than 2^31 rows")
    if isinstance(lambd, bool) or not isinstance(lambd, (int, float)):
        raise ValueError(f"lambd: a number, got {lambd!r}")
    lambd = float(lambd)
    if not (0.0 <= lambd < float("inf")):
        raise ValueError(f"lambd: finite and >= 0, got {lambd!r}")
    return lambd


def _cca_forward(a: Tensor, b: Tensor, lambd: float):
    """The forward export: (terms [4] float64: loss, inv, dec1, dec2; colstat [4 F] float64; gram [2, F, F] float32; the device
    copies of a and b)."""
    dev = _device_for(a)
    with torch.cuda.device(dev):
        d_a = a.detach().to(device=dev).contiguous()
        d_b = b.detach().to(device=dev).contiguous()
        n, f = int(d_a.shape[0]), int(d_a.shape[1])
        out = torch.empty(4 + 4 * f, dtype=torch.float64, device=dev)   # terms | colstat
        gram = torch.empty((2, f, f), dtype=torch.float32, device=dev)
        p = out.data_ptr()
        _device_call("rlap_cca_loss", _lib.CcaInfo, dev, 1, (d_a.data_ptr(), d_b.data_ptr(), n, f, lambd, 0, p, p + 32, gram.data_ptr()))
    return out[:4], out[4:], gram, d_a, d_b


class _CcaLoss(torch.autograd.Function):
    """terms = the fused CCA-SSG loss of (h1, h2) and its three parts; the gradients of the loss with respect to both inputs come
    from the backward export, which reads the forward's column statistics and residuals."""

    @staticmethod
    def forward(ctx, a, b, lambd):
        terms, colstat, gram, d_a, d_b = _cca_forward(a, b, lambd)
        ctx.save_for_backward(d_a, d_b, colstat, gram)
        ctx.call = (lambd, a.device, b.device)
        parts = terms[1:].clone()
        ctx.mark_non_differentiable(parts)
        return terms[0], parts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_parts):
        d_a, d_b, colstat, gram = ctx.saved_tensors
        lambd, dev_a, dev_b = ctx.call
        dev = d_a.device
        with torch.cuda.device(dev):
            d_g = _upstream(g, dev)
            n, f = int(d_a.shape[0]), int(d_a.shape[1])
            ga = torch.empty_like(d_a)
            gb = torch.empty_like(d_b)
            _device_call("rlap_cca_loss_backward", _lib.CcaInfo, dev, 1, (
                d_a.data_ptr(), d_b.data_ptr(), n, f, lambd, 0, colstat.data_ptr(), gram.data_ptr(), d_g.data_ptr(), ga.data_ptr(), gb.data_ptr()))
        return ga.to(dev_a), gb.to(dev_b), None


def cca_loss(h1: Tensor, h2: Tensor, lambd: float = 1e-3, return_terms: bool = False):
    """The CCA-SSG loss of two views' node embeddings, fused on the device (rlap_cca_loss): with
    z = (h - h.mean(0)) / h.std(0), c = z1^T z2 / N, c1 = z1^T z1 / N, c2 = z2^T z2 / N,
    loss = -trace(c) + lambd * (||I - c1||^2 + ||I - c2||^2) -- CCA-SSG/model.py:77-78 and CCA-SSG/main.py:111-124 in one call.

      h1, h2       : (N, F) float32 of equal shape on one device (moved to the library's), N >= 2, F <= 512
      lambd        : the trade-off between invariance and decorrelation, finite and >= 0
      return_terms : return (loss, inv, dec1, dec2), 0-dim float64 each: inv = -trace(c), dec = ||I - c_v||^2 (not differentiable)
    Returns the 0-dim float64 loss.  Every value and the order of every sum are fixed (rlap_amd/csrc/rlap_cca.h): the same input
    gives the same bits.  A column of zero variance gives a NaN loss, as in the reference; nothing is clamped.

    Differentiable in both inputs (rlap_cca_loss_backward standardises again and reads the forward's column statistics and
    residual matrices, it does not repeat the Gram products); double backward is not supported.  Malformed arguments raise
    ValueError before the device is touched.  No host synchronisation.  `last_stats` then holds what the call did
    (rlap_cca_info: rows, features, parts, arena_bytes, host_syncs).
    """
    lambd = _cca_args(h1, h2, lambd)
    if torch.is_grad_enabled() and (h1.requires_grad or h2.requires_grad):
        loss, parts = _CcaLoss.apply(h1, h2, lambd)
    else:
        terms = _cca_forward(h1, h2, lambd)[0]
        loss, parts = terms[0], terms[1:]
    return (loss, parts[0], parts[1], parts[2]) if return_terms else loss


BT_MAX_F = 512
BT_NO_STANDARDIZE = 1   # RLAP_BT_NO_STANDARDIZE


def _bt_number(x, what: str) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise ValueError(f"{what}: a number, got {x!r}")
    x = float(x)
    if not (0.0 <= x < float("inf")):
        raise ValueError(f"{what}: finite and >= 0, got {x!r}")
    return x


def _bt_args(h1, h2, lambd, eps, standardize):
    """Host-side checks of barlow_twins_loss, made before the device is touched: (lambd, eps) as floats and the flags."""
    for t, what in ((h1, "h1"), (h2, "h2")):
        if not isinstance(t, Tensor) or t.dim() != 2:
            raise ValueError(f"{what}: a (num_nodes, F) tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: torch.float32, got {t.dtype}")
    if h1.shape != h2.shape:
        raise ValueError(f"h1 and h2: equal shapes, got {tuple(h1.shape)} and {tuple(h2.shape)}")
    if h1.device != h2.device:
        raise ValueError(f"h1 and h2: one device, got {h1.device} and {h2.device}")
    n, f = int(h1.shape[0]), int(h1.shape[1])
    if n < 2:
        raise ValueError("h1: at least two rows (the unbiased deviation divides by N - 1)")
    if f < 1:
        raise ValueError("h1: at least one feature column")
    if f > BT_MAX_F:
        raise ValueError(f"h1: at most {BT_MAX_F} feature columns, got {f}")
    if n >= 1 << 31:
        raise ValueError("h1: fewer than 2^31 rows")
    if not isinstance(standardize, bool):
        raise ValueError(f"standardize: a bool, got {standardize!r}")
    lambd = 1.0 / f if lambd is None else _bt_number(lambd, "lambd")
    return lambd, _bt_number(eps, "eps"), 0 if standardize else BT_NO_STANDARDIZE


def _bt_forward(a: Tensor, b: Tensor, lambd: float, eps: float, flags: int):
    """The forward export: (terms [3] float64: loss, on, off; colstat [4 F] float64, left as allocated without the standardisation;
    cross (F, F) float32; the device copies of a and b)."""
    dev = _device_for(a)
    with torch.cuda.device(dev):
        d_a = a.detach().to(device=dev).contiguous()
        d_b = b.detach().to(device=dev).contiguous()
        n, f = int(d_a.shape[0]), int(d_a.shape[1])
        out = torch.empty(4 + 4 * f, dtype=torch.float64, device=dev)   # terms (three of four slots) | colstat
        cross = torch.empty((f, f), dtype=torch.float32, device=dev)
        p = out.data_ptr()
        _device_call("rlap_bt_loss", _lib.BtInfo, dev, 1, (d_a.data_ptr(), d_b.data_ptr(), n, f, lambd, eps, flags, p, p + 32, cross.data_ptr()))
    return out[:3], out[4:], cross, d_a, d_b


class _BtLoss(torch.autograd.Function):
    """terms = the fused Barlow Twins loss of (h1, h2) and its two parts; the gradients of the loss with respect to both inputs come
    from the backward export, which reads the forward's column statistics and cross-correlation matrix."""

    @staticmethod
    def forward(ctx, a, b, lambd, eps, flags):
        terms, colstat, cross, d_a, d_b = _bt_forward(a, b, lambd, eps, flags)
        ctx.save_for_backward(d_a, d_b, colstat, cross)
        ctx.call = (lambd, eps, flags, a.device, b.device)
        parts = terms[1:].clone()
        ctx.mark_non_differentiable(parts)
        return terms[0], parts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_parts):
        d_a, d_b, colstat, cross = ctx.saved_tensors
        lambd, eps, flags, dev_a, dev_b = ctx.call
        dev = d_a.device
        with torch.cuda.device(dev):
            d_g = _upstream(g, dev)
            n, f = int(d_a.shape[0]), int(d_a.shape[1])
            ga = torch.empty_like(d_a)
            gb = torch.empty_like(d_b)
            _device_call("rlap_bt_loss_backward", _lib.BtInfo, dev, 1, (
                d_a.data_ptr(), d_b.data_ptr(), n, f, lambd, eps, flags, colstat.data_ptr(), cross.data_ptr(), d_g.data_ptr(), ga.data_ptr(),
                gb.data_ptr()))
        return ga.to(dev_a), gb.to(dev_b), None, None, None


def barlow_twins_loss(h1: Tensor, h2: Tensor, lambd: Optional[float] = None, eps: float = 1e-15, standardize: bool = True,
                      return_terms: bool = False):
    """The Barlow Twins loss of two views' node embeddings, fused on the device (rlap_bt_loss): with
    z = (h - h.mean(0)) / (h.std(0) + eps) and c = z1^T z2 / N,
    loss = sum_k (1 - c_kk)^2 + lambd * sum_{k != l} c_kl^2 -- the published bt_loss of PyGCL's L.BarlowTwins (the G-BT baseline),
    restated: the package is not pinned here.

      h1, h2       : (N, F) float32 of equal shape on one device (moved to the library's), N >= 2, F <= 512
      lambd        : the weight of the off-diagonal term, finite and >= 0; None means 1 / F
      eps          : added to the deviations, finite and >= 0
      standardize  : False takes h1 and h2 as they are (z = h)
      return_terms : return (loss, on, off), 0-dim float64 each: on = sum_k (1 - c_kk)^2, off = sum_{k != l} c_kl^2 (not differentiable)
    Returns the 0-dim float64 loss.  Every value and the order of every sum are fixed (rlap_amd/csrc/rlap_bt.h): the same input
    gives the same bits.  Nothing is clamped: a column of zero variance gives z = 0 and NaN in that column of the gradient (with
    eps = 0 a NaN loss and NaN throughout the other view's gradient too).

    Differentiable in both inputs (rlap_bt_loss_backward standardises again and reads the forward's column statistics and
    cross-correlation matrix, it does not repeat the cross product); double backward is not supported.  Malformed arguments raise
    ValueError before the device is touched.  No host synchronisation.  `last_stats` then holds what the call did
    (rlap_bt_info: rows, features, parts, arena_bytes, host_syncs).
    """
    lambd, eps, flags = _bt_args(h1, h2, lambd, eps, standardize)
    if torch.is_grad_enabled() and (h1.requires_grad or h2.requires_grad):
        loss, parts = _BtLoss.apply(h1, h2, lambd, eps, flags)
    else:
        terms = _bt_forward(h1, h2, lambd, eps, flags)[0]
        loss, parts = terms[0], terms[1:]
    return (loss, parts[0], parts[1]) if return_terms else loss


NORM_MAX_F = _lib.NORM_MAX_F
NORM_PRE = {"none": 0, "relu": _lib.NORM_PRE_RELU}
NORM_POST = {"none": 0, "relu": _lib.NORM_POST_RELU, "prelu": _lib.NORM_POST_PRELU}


def _norm_vector(t, f: int, what: str, x: Tensor):
    if t is None:
        return
    if not isinstance(t, Tensor) or t.dtype != torch.float32 or t.dim() != 1 or int(t.shape[0]) != f:
        raise ValueError(f"{what}: a ({f},) torch.float32 tensor or None")
    if t.device != x.device:
        raise ValueError(f"{what}: on x's device {x.device}, got {t.device}")


def _norm_args(x, weight, bias, running_mean, running_var, training, momentum, eps, pre, post, slope):
    """Host-side checks of batch_norm, made before the device is touched: (flags, momentum, eps)."""
    if not isinstance(x, Tensor) or x.dim() not in (2, 3):
        raise ValueError("x: a (N, F) or (L, N, F) tensor")
    if x.dtype != torch.float32:
        raise ValueError(f"x: torch.float32, got {x.dtype}")
    L, n, f = (1 if x.dim() == 2 else int(x.shape[0])), int(x.shape[-2]), int(x.shape[-1])
    if not isinstance(training, bool):
        raise ValueError(f"training: a bool, got {training!r}")
    if L < 1:
        raise ValueError("x: at least one layer")
    if f < 1 or f > NORM_MAX_F:
        raise ValueError(f"x: between 1 and {NORM_MAX_F} feature columns, got {f}")
    if n < (2 if training else 1):
        raise ValueError("x: at least two rows in training mode (one value per channel has no variance), one in evaluation mode")
    if L * n * f >= 1 << 40:
        raise ValueError("x: fewer than 2^40 elements")
    for t, what in ((weight, "weight"), (bias, "bias"), (running_mean, "running_mean"), (running_var, "running_var")):
        _norm_vector(t, f, what, x)
    if not training and (running_mean is None or running_var is None):
        raise ValueError("running_mean and running_var: both are needed in evaluation mode")
    if momentum is None:
        raise ValueError("momentum: a number in [0, 1]; the cumulative average (momentum=None) is not provided")
    for v, what in ((momentum, "momentum"), (eps, "eps")):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{what}: a number, got {v!r}")
    momentum, eps = float(momentum), float(eps)
    if not (0.0 <= momentum <= 1.0):
        raise ValueError(f"momentum: in [0, 1], got {momentum!r}")
    if not (0.0 < eps < float("inf")):
        raise ValueError(f"eps: finite and > 0, got {eps!r}")
    if not isinstance(pre, str) or pre not in NORM_PRE:
        raise ValueError(f"pre: one of {sorted(NORM_PRE)}, got {pre!r}")
    if not isinstance(post, str) or post not in NORM_POST:
        raise ValueError(f"post: one of {sorted(NORM_POST)}, got {post!r}")
    flags = NORM_PRE[pre] | NORM_POST[post] | (0 if training else _lib.NORM_EVAL)
    if post == "prelu":
        if not isinstance(slope, Tensor) or slope.dtype != torch.float32 or slope.dim() > 1 or slope.numel() not in (1, f):
            raise ValueError(f'slope: with post="prelu" a torch.float32 tensor of one value or of ({f},)')
        if slope.device != x.device:
            raise ValueError(f"slope: on x's device {x.device}, got {slope.device}")
        if slope.numel() == f and f > 1:
            flags |= _lib.NORM_SLOPE_PER_CHANNEL
    elif slope is not None:
        raise ValueError('slope: only with post="prelu"')
    return flags, momentum, eps


def _norm_ptr(t: Optional[Tensor]):
    return t.data_ptr() if t is not None else None


def _norm_forward(x3: Tensor, weight, bias, slope, running_mean, running_var, momentum: float, eps: float, flags: int):
    """The forward export on x3 (L, N, F): (y, stat (L, 3, F) float64 or None in evaluation mode, the device copies of x3, weight,
    bias, slope, running_mean, running_var).  A training call updates the running buffers in place."""
    dev = _device_for(x3)
    with torch.cuda.device(dev):
        put = lambda t: None if t is None else t.detach().to(device=dev).contiguous()
        d_x, d_w, d_b, d_s, d_rm, d_rv = (put(t) for t in (x3, weight, bias, slope, running_mean, running_var))
        L, n, f = (int(v) for v in d_x.shape)
        y = torch.empty_like(d_x)
        stat = None if flags & _lib.NORM_EVAL else torch.empty((L, 3, f), dtype=torch.float64, device=dev)
        _device_call("rlap_batch_norm", _lib.NormInfo, dev, 1, (
            d_x.data_ptr(), L, n, f, _norm_ptr(d_w), _norm_ptr(d_b), _norm_ptr(d_s), _norm_ptr(d_rm), _norm_ptr(d_rv), momentum, eps, flags,
            y.data_ptr(), _norm_ptr(stat)))
        if not flags & _lib.NORM_EVAL:
            with torch.no_grad():
                for buf, d_buf in ((running_mean, d_rm), (running_var, d_rv)):
                    if buf is not None and d_buf.data_ptr() != buf.data_ptr():   # (a copy was updated: a strided or remote buffer)
                        buf.copy_(d_buf)
    return y, stat, (d_x, d_w, d_b, d_s, d_rm, d_rv)


class _BatchNorm(torch.autograd.Function):
    """y = the fused per-view batch norm of x3; the gradients with respect to x, weight, bias and slope come from the backward
    export, which reads x and the forward's column constants `stat` and forms everything else again."""

    @staticmethod
    def forward(ctx, x3, weight, bias, slope, running_mean, running_var, momentum, eps, flags):
        y, stat, (d_x, d_w, d_b, d_s, d_rm, d_rv) = _norm_forward(x3, weight, bias, slope, running_mean, running_var, momentum, eps, flags)
        ev = bool(flags & _lib.NORM_EVAL)
        ctx.save_for_backward(d_x, d_w, d_b, d_s, stat)
        ctx.running = (d_rm, d_rv) if ev else (None, None)
        ctx.call = (eps, flags, [None if t is None else (t.device, t.shape) for t in (x3, weight, bias, slope)])
        if stat is None:
            stat = torch.empty(0, dtype=torch.float64, device=y.device)
        ctx.mark_non_differentiable(stat)
        return y, stat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy, _g_stat):
        d_x, d_w, d_b, d_s, stat = ctx.saved_tensors
        d_rm, d_rv = ctx.running
        eps, flags, origin = ctx.call
        dev = d_x.device
        need = ctx.needs_input_grad
        with torch.cuda.device(dev):
            d_gy = gy.detach().to(device=dev, dtype=torch.float32).contiguous()
            L, n, f = (int(v) for v in d_x.shape)
            gx = torch.empty_like(d_x) if need[0] else None
            gw = torch.empty(f, dtype=torch.float32, device=dev) if need[1] and d_w is not None else None
            gb = torch.empty(f, dtype=torch.float32, device=dev) if need[2] and d_b is not None else None
            gs = torch.empty(d_s.numel(), dtype=torch.float32, device=dev) if need[3] and d_s is not None else None
            _device_call("rlap_batch_norm_backward", _lib.NormInfo, dev, 1, (
                d_x.data_ptr(), d_gy.data_ptr(), L, n, f, _norm_ptr(d_w), _norm_ptr(d_b), _norm_ptr(d_s), _norm_ptr(d_rm), _norm_ptr(d_rv),
                eps, flags, _norm_ptr(stat), _norm_ptr(gx), _norm_ptr(gw), _norm_ptr(gb), _norm_ptr(gs)))
        back = lambda g, o: None if g is None else g.reshape(o[1]).to(o[0])
        return (back(gx, origin[0]), back(gw, origin[1]), back(gb, origin[2]), back(gs, origin[3]), None, None, None, None, None)


def batch_norm(x: Tensor, weight: Optional[Tensor] = None, bias: Optional[Tensor] = None, running_mean: Optional[Tensor] = None,
               running_var: Optional[Tensor] = None, training: bool = True, momentum: float = 0.1, eps: float = 1e-5, pre: str = "none",
               post: str = "none", slope: Optional[Tensor] = None, return_stats: bool = False):
    """Batch norm of every view on its own, with the activations around it fused in (rlap_batch_norm):
    y[l] = post(F.batch_norm(pre(x[l]), running_mean, running_var, weight, bias, training, momentum, eps)) for every layer l of an
    (L, N, F) tensor in one call -- what the reference's encoders compute by running once per view: each view is normalised with
    its own batch statistics, and the running buffers are updated once per view, in view order.

      x            : (N, F) or (L, N, F) float32; 1 <= F <= 4096; N >= 2 in training mode
      weight, bias : (F,) float32 or None (1 and 0)
      running_mean, running_var : (F,) float32 or None; updated in place in training mode (rm = (1 - momentum) rm + momentum mean,
                     rv the same with the unbiased variance, layer 0 first), read in evaluation mode, where both are needed
      momentum     : in [0, 1]; None (torch's cumulative average) is not provided
      pre          : "none" or "relu", applied to x in front of the norm
      post         : "none", "relu" or "prelu", applied behind it; "prelu" takes `slope`, one float32 value or (F,) per channel
      return_stats : also return (mean, var), float64 (L, F): every layer's batch mean and biased variance (var is recovered from
                     the stored 1 / sqrt(var + eps)); in evaluation mode the running buffers
    Returns y of x's shape.  Every value and the order of every sum are fixed (rlap_amd/csrc/rlap_norm.h: float64, the column sums
    by the chunk rule, one rounding to float32): the same input gives the same bits, forward and backward, and layer l of a call
    equals the (N, F) call on x[l] alone.  A column of zero variance gives 1 / sqrt(eps), no NaN.

    Differentiable in x, weight, bias and slope (rlap_batch_norm_backward; nothing of x's size but x itself is kept for it); double
    backward is not supported.  Malformed arguments raise ValueError before the device is touched.  No host synchronisation.
    `last_stats` then holds what the call did (rlap_norm_info: rows, features, layers, chunks, arena_bytes, vec -- 1 when the rows
    were read 16 bytes a lane --, launches, host_syncs).
    """
    flags, momentum, eps = _norm_args(x, weight, bias, running_mean, running_var, training, momentum, eps, pre, post, slope)
    x3 = x if x.dim() == 3 else x.unsqueeze(0)
    params = (x, weight, bias, slope)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in params):
        y, stat = _BatchNorm.apply(x3, weight, bias, slope, running_mean, running_var, momentum, eps, flags)
    else:
        y, stat, _ = _norm_forward(x3, weight, bias, slope, running_mean, running_var, momentum, eps, flags)
    y = y if x.dim() == 3 else y.squeeze(0)
    if not return_stats:
        return y
    if training:
        s = stat.detach()
        return y, s[:, 0] + s[:, 1], (s[:, 2].reciprocal().square() - eps).clamp_min(0.0)
    L = int(x3.shape[0])
    return y, running_mean.detach().double().expand(L, -1).to(y.device), running_var.detach().double().expand(L, -1).to(y.device)


ROW_MAX_F = _lib.ROW_MAX_F
ROW_ACT = {"none": 0, "relu": _lib.ROW_ACT_RELU, "prelu": _lib.ROW_ACT_PRELU}


def _row_args(x, vectors, act, slope, p, training, seed, what_act: str):
    """Host-side checks of bias_act_dropout and layer_norm, made before the device is touched: (flags, p, seed)."""
    if not isinstance(x, Tensor) or x.dim() not in (2, 3):
        raise ValueError("x: a (N, F) or (L, N, F) tensor")
    if x.dtype != torch.float32:
        raise ValueError(f"x: torch.float32, got {x.dtype}")
    L, n, f = (1 if x.dim() == 2 else int(x.shape[0])), int(x.shape[-2]), int(x.shape[-1])
    if not isinstance(training, bool):
        raise ValueError(f"training: a bool, got {training!r}")
    if L < 1 or n < 1:
        raise ValueError("x: at least one layer and one row")
    if f < 1 or f > ROW_MAX_F:
        raise ValueError(f"x: between 1 and {ROW_MAX_F} feature columns, got {f}")
    if L * n * f >= 1 << 40:
        raise ValueError("x: fewer than 2^40 elements")
    for t, what in vectors:
        _norm_vector(t, f, what, x)
    if isinstance(p, bool) or not isinstance(p, (int, float)):
        raise ValueError(f"p: a number, got {p!r}")
    p = float(p)
    if not (0.0 <= p < 1.0):
        raise ValueError(f"p: in [0, 1), got {p!r}")
    if not isinstance(act, str) or act not in ROW_ACT:
        raise ValueError(f"{what_act}: one of {sorted(ROW_ACT)}, got {act!r}")
    flags = ROW_ACT[act] | (_lib.ROW_TRAINING if training else 0)
    if act == "prelu":
        if not isinstance(slope, Tensor) or slope.dtype != torch.float32 or slope.dim() > 1 or slope.numel() not in (1, f):
            raise ValueError(f'slope: with {what_act}="prelu" a torch.float32 tensor of one value or of ({f},)')
        if slope.device != x.device:
            raise ValueError(f"slope: on x's device {x.device}, got {slope.device}")
        if slope.numel() == f and f > 1:
            flags |= _lib.ROW_SLOPE_PER_CHANNEL
    elif slope is not None:
        raise ValueError(f'slope: only with {what_act}="prelu"')
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
        raise ValueError(f"seed: an int or None, got {seed!r}")
    dropping = training and p > 0.0
    return flags, p, (_seed_from(seed) if dropping or seed is not None else 0)


def _row_forward(export: str, x3: Tensor, params: tuple, head: tuple, p: float, seed: int, flags: int):
    """The forward export `export` on x3 (L, N, F): (y, the device copies of x3 and of `params`).  `head` holds the scalar
    arguments between the parameters and p."""
    dev = _device_for(x3)
    with torch.cuda.device(dev):
        put = lambda t: None if t is None else t.detach().to(device=dev).contiguous()
        d_x = put(x3)
        d_params = tuple(put(t) for t in params)
        L, n, f = (int(v) for v in d_x.shape)
        y = torch.empty_like(d_x)
        _device_call(export, _lib.RowopsInfo, dev, 1, (d_x.data_ptr(), L, n, f, *(_norm_ptr(t) for t in d_params), *head, p, seed, flags, y.data_ptr()))
    return y, d_x, d_params


class _RowPass(torch.autograd.Function):
    """y = the fused row pass `export` of x3; the gradients with respect to x and the parameters come from the backward export,
    which reads x and draws the forward's dropout coins again from (p, seed): nothing but x is kept."""

    @staticmethod
    def forward(ctx, export, head, p, seed, flags, x3, *params):
        y, d_x, d_params = _row_forward(export, x3, params, head, p, seed, flags)
        ctx.save_for_backward(d_x, *[t for t in d_params if t is not None])
        ctx.present = [t is not None for t in d_params]
        ctx.call = (export, head, p, seed, flags, [None if t is None else (t.device, t.shape) for t in (x3, *params)])
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        saved = list(ctx.saved_tensors)
        d_x = saved.pop(0)
        d_params = [saved.pop(0) if here else None for here in ctx.present]
        export, head, p, seed, flags, origin = ctx.call
        dev = d_x.device
        need = ctx.needs_input_grad[5:]
        with torch.cuda.device(dev):
            d_gy = gy.detach().to(device=dev, dtype=torch.float32).contiguous()
            L, n, f = (int(v) for v in d_x.shape)
            gx = torch.empty_like(d_x) if need[0] else None
            grads = [torch.empty(t.numel(), dtype=torch.float32, device=dev) if t is not None and need[1 + k] else None
                     for k, t in enumerate(d_params)]
            _device_call(export + "_backward", _lib.RowopsInfo, dev, 1, (
                d_x.data_ptr(), d_gy.data_ptr(), L, n, f, *(_norm_ptr(t) for t in d_params), *head, p, seed, flags,
                _norm_ptr(gx), *(_norm_ptr(g) for g in grads)))
        back = lambda g, o: None if g is None else g.reshape(o[1]).to(o[0])
        return (None, None, None, None, None, back(gx, origin[0])) + tuple(back(g, o) for g, o in zip(grads, origin[1:]))


def _row_call(export: str, x: Tensor, params: tuple, head: tuple, p: float, seed: int, flags: int) -> Tensor:
    x3 = x if x.dim() == 3 else x.unsqueeze(0)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, *params)):
        y = _RowPass.apply(export, head, p, seed, flags, x3, *params)
    else:
        y = _row_forward(export, x3, params, head, p, seed, flags)[0]
    return y if x.dim() == 3 else y.squeeze(0)


def bias_act_dropout(x: Tensor, bias: Optional[Tensor] = None, act: str = "none", slope: Optional[Tensor] = None, p: float = 0.0,
                     training: bool = True, seed: Optional[int] = 0) -> Tensor:
    """y = F.dropout(act(x + bias), p, training) in one pass over x (rlap_bias_act_dropout) -- the bias add, the PReLU
    and the dropout that the reference's encoders run behind every GCN and GIN layer, 8 bytes an element instead of three passes,
    and no mask kept: the dropout coin is a function of (seed, layer, row, column, F, p) alone and is drawn again in the backward pass.

      x        : (N, F) or (L, N, F) float32; 1 <= F <= 4096
      bias     : (F,) float32 or None (0)
      act      : "none", "relu" or "prelu"; "prelu" takes `slope`, one float32 value or (F,) per channel
      p        : the drop probability, 0 <= p < 1; used as T / 65536 with T = round(p * 65536), and what is kept is scaled by
                 1 / (1 - T / 65536)
      training : False switches the dropout off, as p = 0 does: the call then gives the bits of the call without dropout
      seed     : an int fixes the mask; None draws one seed from torch's generator, as drop_edges does.  Layer l of an (L, N, F)
                 call draws the coins of the (N, F) call with seed + l.
    Returns y of x's shape.  Every value is fixed (rlap_amd/csrc/rlap_rowops.h: float64, one rounding to float32): the same input
    and seed give the same bits, forward and backward, on either lane path.

    Differentiable in x, bias and slope (rlap_bias_act_dropout_backward, with the saved seed); double backward is not supported.
    Malformed arguments raise ValueError before the device is touched.  No host synchronisation.  `last_stats` then holds what
    the call did (rlap_rowops_info: rows, features, layers, chunks, arena_bytes, vec, launches, instance, host_syncs).
    """
    flags, p, seed = _row_args(x, ((bias, "bias"),), act, slope, p, training, seed, "act")
    return _row_call("rlap_bias_act_dropout", x, (bias, slope), (), p, seed, flags)


def layer_norm(x: Tensor, weight: Optional[Tensor] = None, bias: Optional[Tensor] = None, eps: float = 1e-5, post: str = "none",
               slope: Optional[Tensor] = None, p: float = 0.0, training: bool = True, seed: Optional[int] = 0) -> Tensor:
    """y = F.dropout(post(F.layer_norm(x, (F,), weight, bias, eps)), p, training) in one pass (rlap_layer_norm): every
    row of an (N, F) or (L, N, F) float32 tensor is normalised over its F columns -- the LayerNorm branch of the reference's
    Normalize with the PReLU and the dropout behind it.  A wave holds the row; x is read once and y written once.

      weight, bias : (F,) float32 or None (1 and 0)
      eps          : finite and > 0; a constant row gives 1 / sqrt(eps), no NaN
      post, slope, p, training, seed : as bias_act_dropout's act, slope, p, training and seed
    The row sums run in an order that depends on F alone (rlap_amd/csrc/rlap_rowops.h), so the same input gives the same bits on
    either lane path.  Differentiable in x, weight, bias and slope (rlap_layer_norm_backward; nothing but x is kept for it).
    Malformed arguments raise ValueError before the device is touched.  No host synchronisation.  `last_stats` as
    bias_act_dropout; `instance` is the number of 16-byte steps a lane takes over a row (1, 2, 4: in registers; 8, 16: through LDS).
    """
    flags, p, seed = _row_args(x, ((weight, "weight"), (bias, "bias")), post, slope, p, training, seed, "post")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (0.0 < float(eps) < float("inf")):
        raise ValueError(f"eps: finite and > 0, got {eps!r}")
    return _row_call("rlap_layer_norm", x, (weight, bias, slope), (float(eps),), p, seed, flags)


LINEAR_MAX_F = _lib.LINEAR_MAX_F
LINEAR_ACT = {"none": _lib.LINEAR_ACT_NONE, "relu": _lib.LINEAR_ACT_RELU, "elu": _lib.LINEAR_ACT_ELU}
LINEAR_LAYOUT = {"in_out": 0, "out_in": _lib.LINEAR_WEIGHT_OUT_IN}


def _linear_args(x, weight, bias, act, alpha, weight_layout):
    """Host-side checks of linear_act, made before the device is touched: (act code, alpha, flags, Fin, Fout)."""
    if not isinstance(x, Tensor) or x.dim() not in (2, 3):
        raise ValueError("x: a (N, Fin) or (L, N, Fin) tensor")
    if x.dtype != torch.float32:
        raise ValueError(f"x: torch.float32, got {x.dtype}")
    if not isinstance(weight_layout, str) or weight_layout not in LINEAR_LAYOUT:
        raise ValueError(f"weight_layout: one of {sorted(LINEAR_LAYOUT)}, got {weight_layout!r}")
    if not isinstance(weight, Tensor) or weight.dim() != 2:
        raise ValueError("weight: a (Fin, Fout) tensor, or (Fout, Fin) with weight_layout=\"out_in\"")
    if weight.dtype != torch.float32:
        raise ValueError(f"weight: torch.float32, got {weight.dtype}")
    if weight.device != x.device:
        raise ValueError(f"weight: on x's device {x.device}, got {weight.device}")
    flags = LINEAR_LAYOUT[weight_layout]
    fin, fout = (int(weight.shape[1]), int(weight.shape[0])) if flags else (int(weight.shape[0]), int(weight.shape[1]))
    rows = int(x.shape[-2]) * (1 if x.dim() == 2 else int(x.shape[0]))
    if rows < 1:
        raise ValueError("x: at least one layer and one row")
    if rows >= 1 << 31:
        raise ValueError("x: fewer than 2^31 rows in all")
    if int(x.shape[-1]) != fin:
        raise ValueError(f"x: {fin} feature columns as the weight's, got {int(x.shape[-1])}")
    for f, what in ((fin, "Fin"), (fout, "Fout")):
        if f < 1 or f > LINEAR_MAX_F:
            raise ValueError(f"{what}: between 1 and {LINEAR_MAX_F}, got {f}")
    if bias is not None:
        if not isinstance(bias, Tensor) or bias.dtype != torch.float32 or bias.dim() != 1 or int(bias.shape[0]) != fout:
            raise ValueError(f"bias: a ({fout},) torch.float32 tensor or None")
        if bias.device != x.device:
            raise ValueError(f"bias: on x's device {x.device}, got {bias.device}")
    if not isinstance(act, str) or act not in LINEAR_ACT:
        raise ValueError(f"act: one of {sorted(LINEAR_ACT)}, got {act!r}")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not (0.0 < float(alpha) < float("inf")):
        raise ValueError(f"alpha: finite and > 0, got {alpha!r}")
    return LINEAR_ACT[act], float(alpha), flags, fin, fout


def _linear_forward(x: Tensor, weight: Tensor, bias: Optional[Tensor], act: int, alpha: float, flags: int, fin: int, fout: int):
    """The forward export on x (..., Fin): (y (..., Fout), the device copies of x, weight and bias)."""
    dev = _device_for(x)
    with torch.cuda.device(dev):
        put = lambda t: None if t is None else t.detach().to(device=dev).contiguous()
        d_x, d_w, d_b = put(x), put(weight), put(bias)
        rows = d_x.numel() // fin
        y = torch.empty(tuple(d_x.shape[:-1]) + (fout,), dtype=torch.float32, device=dev)
        _device_call("rlap_linear_act", _lib.LinearInfo, dev, 1, (
            d_x.data_ptr(), rows, fin, fout, d_w.data_ptr(), _norm_ptr(d_b), act, alpha, flags, y.data_ptr()))
    return y, d_x, d_w, d_b


class _LinearAct(torch.autograd.Function):
    """y = act(x W + b) by the fused dense layer; the gradients that are required come from the backward export, which reads x, W
    and y: the pre-activation is never kept."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, alpha, flags, fin, fout):
        y, d_x, d_w, d_b = _linear_forward(x, weight, bias, act, alpha, flags, fin, fout)
        ctx.save_for_backward(d_x, d_w, y)
        ctx.call = (act, alpha, flags, fin, fout, x.device, weight.device, None if bias is None else bias.device)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        d_x, d_w, y = ctx.saved_tensors
        act, alpha, flags, fin, fout, dev_x, dev_w, dev_b = ctx.call
        dev = d_x.device
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], dev_b is not None and ctx.needs_input_grad[2]
        with torch.cuda.device(dev):
            d_gy = gy.detach().to(device=dev, dtype=torch.float32).contiguous()
            gx = torch.empty_like(d_x) if need_x else None
            gw = torch.empty_like(d_w) if need_w else None
            gb = torch.empty(fout, dtype=torch.float32, device=dev) if need_b else None
            _device_call("rlap_linear_act_backward", _lib.LinearInfo, dev, 1, (
                d_x.data_ptr(), d_w.data_ptr(), y.data_ptr(), d_gy.data_ptr(), d_x.numel() // fin, fin, fout, act, alpha, flags,
                _norm_ptr(gx), _norm_ptr(gw), _norm_ptr(gb)))
        back = lambda g, d: None if g is None else g.to(d)
        return back(gx, dev_x), back(gw, dev_w), back(gb, dev_b), None, None, None, None, None


def linear_act(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, act: str = "none", alpha: float = 1.0,
               weight_layout: str = "in_out") -> Tensor:
    """y = act(x @ W + bias) in one pass over x (rlap_linear_act) -- the torch.nn.Linear and the elementwise launches
    behind it of the encoders, the GIN layers' MLP and the projection heads: the bias and the activation are applied to the
    accumulator, x is read once and y written once, and nothing but x, W and y is kept for the backward pass.

      x             : (N, Fin) or (L, N, Fin) float32; 1 <= Fin <= 512.  The layers share the weight: the call is the (L N, Fin) one.
      weight        : (Fin, Fout) float32, 1 <= Fout <= 512; with weight_layout="out_in" (Fout, Fin), torch.nn.Linear's layout
                      (no transposed copy is made)
      bias          : (Fout,) float32 or None
      act           : "none", "relu" or "elu"; `alpha` is ELU's, finite and > 0
    Returns y of x's leading shape, (..., Fout).  Every value and the order of every sum are fixed (rlap_amd/csrc/rlap_linear.h:
    float32 fmaf chains over the inner index, what the f32 matrix-core instruction computes; bias, activation and one rounding in
    float64): the same input gives the same bits, however the tensors are aligned.

    Differentiable in x, weight and bias (rlap_linear_act_backward; only the gradients that are required are computed); double
    backward is not supported.  Malformed arguments raise ValueError before the device is touched.  No host synchronisation.
    `last_stats` then holds what the call did (rlap_linear_info: rows, fin, fout, parts, arena_bytes, host_syncs).
    """
    args = _linear_args(x, weight, bias, act, alpha, weight_layout)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias)):
        return _LinearAct.apply(x, weight, bias, *args)
    return _linear_forward(x, weight, bias, *args)[0]


G2L_MAX_F = 512


def _g2l_args(h, g, node_ptr, neg, what_neg: bool):
    """Host-side checks of g2l_jsd / g2l_bootstrap, made before the device is touched: the GraphTable of the call."""
    tensors = [(h, "h"), (g, "g")] + ([(neg, "neg")] if neg is not None else [])
    for t, what in tensors:
        if not isinstance(t, Tensor) or t.dim() != 2:
            raise ValueError(f"{what}: a (rows, F) tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: torch.float32, got {t.dtype}")
    n, f, G = int(h.shape[0]), int(h.shape[1]), int(g.shape[0])
    if n < 1 or f < 1:
        raise ValueError("h: at least one row and one feature column")
    if G < 1:
        raise ValueError("g: at least one graph")
    if int(g.shape[1]) != f:
        raise ValueError(f"h and g: the same number of feature columns, got {f} and {int(g.shape[1])}")
    if f > G2L_MAX_F:
        raise ValueError(f"h: at most {G2L_MAX_F} feature columns, got {f}")
    if n >= 1 << 31 or G >= 1 << 31:
        raise ValueError("h, g: fewer than 2^31 rows")
    if neg is not None and neg.shape != h.shape:
        raise ValueError(f"h and neg: equal shapes, got {tuple(h.shape)} and {tuple(neg.shape)}")
    if node_ptr is None:
        if G != 1:
            raise ValueError(f"node_ptr: required for g of {G} graphs (the default [0, N] is one graph)")
        node_ptr = [0, n]
    table = _graph_table(node_ptr, n)
    if table.graphs != G:
        raise ValueError(f"node_ptr: {table.graphs} graphs, g has {G} rows")
    if what_neg:
        if G == 1 and neg is None:
            raise ValueError("neg: required for one graph (the embeddings of the corrupted input are its negatives)")
        if G >= 2 and neg is not None:
            raise ValueError("neg: only for one graph (with several, the other graphs' summaries are the negatives)")
    return table


def _g2l_jsd_forward(h: Tensor, g: Tensor, neg: Optional[Tensor], table: GraphTable):
    """The forward export: (loss 0-dim, rows (2, N): pos_i, neg_i; the device copies of h, g, neg)."""
    dev = _device_for(h)
    with torch.cuda.device(dev):
        d_h = h.detach().to(device=dev).contiguous()
        d_g = g.detach().to(device=dev).contiguous()
        d_n = neg.detach().to(device=dev).contiguous() if neg is not None else None
        n, f = int(d_h.shape[0]), int(d_h.shape[1])
        out = torch.empty(1 + 2 * n, dtype=torch.float64, device=dev)   # loss | pos | neg
        p = out.data_ptr()
        _device_call("rlap_g2l_jsd", _lib.G2lInfo, dev, table.graphs, (
            d_h.data_ptr(), d_n.data_ptr() if d_n is not None else None, d_g.data_ptr(), n, f, table.on(dev).data_ptr(), table.graphs, 0, p, p + 8))
    return out[0], out[1:].view(2, n), d_h, d_g, d_n


class _G2lJsd(torch.autograd.Function):
    """loss = the fused JSD of (h, g) in the graph-to-local mode; the gradients with respect to h, g and neg come from the backward
    export, which recomputes the scores."""

    @staticmethod
    def forward(ctx, h, g, neg, table):
        loss, rows, d_h, d_g, d_n = _g2l_jsd_forward(h, g, neg, table)
        ctx.save_for_backward(d_h, d_g, *([d_n] if d_n is not None else []))
        ctx.call = (table, h.device, g.device, neg.device if neg is not None else None)
        ctx.mark_non_differentiable(rows)
        return loss, rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gup, _g_rows):
        d_h, d_g = ctx.saved_tensors[:2]
        d_n = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        table, dev_h, dev_g, dev_n = ctx.call
        dev = d_h.device
        with torch.cuda.device(dev):
            d_up = _upstream(gup, dev)
            n, f = int(d_h.shape[0]), int(d_h.shape[1])
            gh, gg = torch.empty_like(d_h), torch.empty_like(d_g)
            gn = torch.empty_like(d_n) if d_n is not None else None
            _device_call("rlap_g2l_jsd_backward", _lib.G2lInfo, dev, table.graphs, (
                d_h.data_ptr(), d_n.data_ptr() if d_n is not None else None, d_g.data_ptr(), n, f, table.on(dev).data_ptr(), table.graphs, 0,
                d_up.data_ptr(), gh.data_ptr(), gn.data_ptr() if gn is not None else None, gg.data_ptr()))
        return gh.to(dev_h), gg.to(dev_g), gn.to(dev_n) if gn is not None else None, None


def g2l_jsd(h: Tensor, g: Tensor, node_ptr: Union[Tensor, Sequence[int], GraphTable, None] = None, neg: Optional[Tensor] = None,
            return_rows: bool = False):
    """The Jensen-Shannon contrastive loss between node embeddings and graph summaries, fused on the device (rlap_g2l_jsd, DESIGN
    4.17): one direction of DualBranchContrast(JSD(), mode="G2L") of scripts/node_dedicated.py.  The JSD loss and the mode's branches
    are the reference's text (scripts/node_dedicated.py: JSD.compute; scripts/node_shared.py: DualBranchContrast.forward); the masks
    restate PyGCL's published CrossScaleSampler, which is not installed here.  With s_ij = <h_i, g_j> and g(i) the graph of node i:
    the positives are the pairs (i, g(i)); with several graphs the negatives are every (i, j), j != g(i); with one graph they are
    s'_i = <neg_i, g_0>;  loss = mean_neg(softplus(s) - ln 2) - mean_pos(ln 2 - softplus(-s)).

      h           : (N, F) float32 node embeddings, F <= 512, on any device (moved to the library's)
      g           : (G, F) float32 graph summaries
      node_ptr    : [G+1] offsets, non-decreasing from 0 to N, checked on the host, or an ops.GraphTable; None is [0, N], one graph.
                    Empty graphs and G > N are legal.
      neg         : (N, F) float32, the embeddings of the corrupted input: required for one graph, refused for several
      return_rows : also return the (2, N) float64 row terms: pos_i, and neg_i, the sum of node i's negative terms (not
                    differentiable)
    Returns the 0-dim float64 loss.  Every value and the order of every sum are fixed (rlap_amd/csrc/rlap_g2l.h): the same input
    gives the same bits.  No (2N, F) copy, no (G, N) mask or similarity matrix is formed.

    Differentiable in h, g and neg (rlap_g2l_jsd_backward); double backward is not supported.  Malformed arguments raise ValueError
    before the device is touched; a score that is not finite gives a NaN loss.  No host synchronisation.  `last_stats` then holds what
    the call did (rlap_g2l_info: rows, graphs, features, parts, arena_bytes, host_syncs).
    """
    table = _g2l_args(h, g, node_ptr, neg, True)
    if torch.is_grad_enabled() and (h.requires_grad or g.requires_grad or (neg is not None and neg.requires_grad)):
        loss, rows = _G2lJsd.apply(h, g, neg, table)
    else:
        loss, rows = _g2l_jsd_forward(h, g, neg, table)[:2]
    return (loss, rows) if return_rows else loss


def _g2l_bootstrap_forward(h: Tensor, g: Tensor, table: GraphTable):
    """The forward export: (loss 0-dim, rows [N]: c_i; the device copies of h and g)."""
    dev = _device_for(h)
    with torch.cuda.device(dev):
        d_h = h.detach().to(device=dev).contiguous()
        d_g = g.detach().to(device=dev).contiguous()
        n, f = int(d_h.shape[0]), int(d_h.shape[1])
        out = torch.empty(1 + n, dtype=torch.float64, device=dev)   # loss | c
        p = out.data_ptr()
        _device_call("rlap_g2l_bootstrap", _lib.G2lInfo, dev, table.graphs, (
            d_h.data_ptr(), d_g.data_ptr(), n, f, table.on(dev).data_ptr(), table.graphs, 0, p, p + 8))
    return out[0], out[1:], d_h, d_g


class _G2lBootstrap(torch.autograd.Function):
    """loss = the fused bootstrap loss of (h, g) in the graph-to-local mode; the gradient with respect to h comes from the backward
    export.  g is a constant."""

    @staticmethod
    def forward(ctx, h, g, table):
        loss, rows, d_h, d_g = _g2l_bootstrap_forward(h, g, table)
        ctx.save_for_backward(d_h, d_g)
        ctx.call = (table, h.device)
        ctx.mark_non_differentiable(rows)
        return loss, rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gup, _g_rows):
        d_h, d_g = ctx.saved_tensors
        table, dev_h = ctx.call
        dev = d_h.device
        with torch.cuda.device(dev):
            d_up = _upstream(gup, dev)
            n, f = int(d_h.shape[0]), int(d_h.shape[1])
            gh = torch.empty_like(d_h)
            _device_call("rlap_g2l_bootstrap_backward", _lib.G2lInfo, dev, table.graphs, (
                d_h.data_ptr(), d_g.data_ptr(), n, f, table.on(dev).data_ptr(), table.graphs, 0, d_up.data_ptr(), gh.data_ptr()))
        return gh.to(dev_h), None, None


def g2l_bootstrap(h: Tensor, g: Tensor, node_ptr: Union[Tensor, Sequence[int], GraphTable, None] = None, return_rows: bool = False):
    """The bootstrap loss between node predictions and graph targets, fused on the device (rlap_g2l_bootstrap): one
    direction of BootstrapContrast(BootstrapLatent(), mode="G2L") of scripts/graph_shared_g2l.py.  PyGCL is not installed here: this
    restates its published BootstrapLatent and BootstrapContrast.  With the rows of h and g normalised as F.normalize does and g(i)
    the graph of node i:  loss = (sum_i cos(h_i, g_{g(i)})) / G, the mean over graphs of the per-graph sums of cosines.  The sign is
    PyGCL's as published: the sum is not negated.

      h           : (N, F) float32 node predictions, F <= 512, on any device (moved to the library's)
      g           : (G, F) float32 graph targets; a constant (the script detaches them): a g that requires grad raises ValueError
      node_ptr    : [G+1] offsets, non-decreasing from 0 to N, checked on the host, or an ops.GraphTable; None is [0, N], one graph
      return_rows : also return the (N,) float64 cosines c_i (not differentiable)
    Returns the 0-dim float64 loss.  Every value and the order of every sum are fixed (rlap_amd/csrc/rlap_g2l.h): the same input
    gives the same bits.

    Differentiable in h (rlap_g2l_bootstrap_backward); double backward is not supported.  Malformed arguments raise ValueError before
    the device is touched.  No host synchronisation.  `last_stats` then holds what the call did (rlap_g2l_info).
    """
    table = _g2l_args(h, g, node_ptr, None, False)
    if g.requires_grad:
        raise ValueError("g: the bootstrap targets are constants; detach them (there is no gradient for g)")
    if torch.is_grad_enabled() and h.requires_grad:
        loss, rows = _G2lBootstrap.apply(h, g, table)
    else:
        loss, rows = _g2l_bootstrap_forward(h, g, table)[:2]
    return (loss, rows) if return_rows else loss


PLAN_DIRECTIONS = {"forward": _lib.PLAN_FORWARD, "transposed": _lib.PLAN_TRANSPOSED, "both": _lib.PLAN_FORWARD | _lib.PLAN_TRANSPOSED}


PROBE_MAX_F, PROBE_MAX_C, PROBE_MAX_RUNS = 512, 64, 32
PROBE_SELECT = {"scripts": _lib.PROBE_SELECT_SCRIPTS, "cca": _lib.PROBE_SELECT_CCA}


def _probe_lists(arg, what: str) -> Tuple[Tensor, list]:
    """The runs' index lists of linear_probe / probe_scores as (concatenated int64 indices, the [R+1] offsets as Python ints), from
    an index tensor (one run), a list of index tensors (ragged) or a tuple (indices, ptr) whose ptr lives on the host."""
    if isinstance(arg, tuple):
        if len(arg) != 2:
            raise ValueError(f"{what}: an index tensor, a list of index tensors or a tuple (indices, ptr)")
        flat, ptr = arg
        if isinstance(ptr, Tensor):
            if ptr.is_cuda:
                raise ValueError(f"{what}: ptr on the host (a CPU tensor or a sequence of ints); reading it from the device would synchronise")
            ptr = ptr.tolist()
        ptr = [int(p) for p in ptr]
        if not isinstance(flat, Tensor) or flat.dim() != 1 or flat.dtype != torch.int64:
            raise ValueError(f"{what}: indices as a 1-D torch.int64 tensor")
        if len(ptr) < 2 or ptr[0] != 0 or ptr[-1] != flat.numel():
            raise ValueError(f"{what}: ptr runs from 0 to the number of indices")
    else:
        lists = [arg] if isinstance(arg, Tensor) else list(arg) if isinstance(arg, (list,)) else None
        if not lists:
            raise ValueError(f"{what}: an index tensor, a list of index tensors or a tuple (indices, ptr)")
        for t in lists:
            if not isinstance(t, Tensor) or t.dim() != 1 or t.dtype != torch.int64:
                raise ValueError(f"{what}: every index list a 1-D torch.int64 tensor")
        ptr = [0]
        for t in lists:
            ptr.append(ptr[-1] + int(t.numel()))
        flat = lists[0] if len(lists) == 1 else torch.cat([t.to(lists[0].device) for t in lists])
    if any(b <= a for a, b in zip(ptr[:-1], ptr[1:])):
        raise ValueError(f"{what}: every set of every run must be non-empty")
    return flat, ptr


def _probe_inputs(x, y, num_classes):
    """Host-side checks of x, y and the class count; C from y.max() when it is not given (the one host read before the call)."""
    if not isinstance(x, Tensor) or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("x: a (N, F) torch.float32 tensor")
    if not isinstance(y, Tensor) or y.dim() != 1 or y.dtype != torch.int64 or y.shape[0] != x.shape[0]:
        raise ValueError("y: a (N,) torch.int64 tensor, one label per row of x")
    n, f = int(x.shape[0]), int(x.shape[1])
    if n < 1 or n >= 1 << 31:
        raise ValueError("x: between 1 and 2^31 - 1 rows")
    if not 1 <= f <= PROBE_MAX_F:
        raise ValueError(f"x: between 1 and {PROBE_MAX_F} feature columns, got {f}")
    c = int(y.max()) + 1 if num_classes is None else int(num_classes)
    if not 2 <= c <= PROBE_MAX_C:
        raise ValueError(f"num_classes: between 2 and {PROBE_MAX_C}, got {c}")
    return n, f, c


def _probe_x(x: Tensor, dev) -> Tuple[Tensor, int]:
    """x on the library's device and its row stride: a view with unit column stride and rows at least F apart is read in place,
    anything else is copied."""
    d_x = x.detach().to(device=dev)
    n, f = int(d_x.shape[0]), int(d_x.shape[1])
    unit = f == 1 or d_x.stride(1) == 1
    if not unit or (n > 1 and d_x.stride(0) < f):
        d_x = d_x.contiguous()
    return d_x, (int(d_x.stride(0)) if n > 1 else f)


def probe_init(num_runs: int, num_classes: int, num_features: int, generator=None) -> Tuple[Tensor, Tensor]:
    """The initial parameters of `num_runs` probes as the reference draws them (scripts/node_shared.py:152-156), on the host:
    nn.Linear's default draws (a weight that is thrown away, the bias in U(-1/sqrt(F), 1/sqrt(F))) and then xavier_uniform_ for the
    weight, U(-a, a) with a = sqrt(6 / (F + C)) -- in that order, so a generator seeded as the reference's yields its values.
    Returns ((R, C, F), (R, C)) float32."""
    r, c, f = int(num_runs), int(num_classes), int(num_features)
    w = torch.empty((r, c, f), dtype=torch.float32)
    b = torch.empty((r, c), dtype=torch.float32)
    kb = 1.0 / f ** 0.5
    xa = (6.0 / (f + c)) ** 0.5
    for k in range(r):
        w[k].uniform_(-kb, kb, generator=generator)
        b[k].uniform_(-kb, kb, generator=generator)
        w[k].uniform_(-xa, xa, generator=generator)
    return w, b


def _i64_array(values):
    return (ctypes.c_int64 * len(values))(*values)


def linear_probe(x: Tensor, y: Tensor, train, valid, test, num_classes: Optional[int] = None, epochs: int = 2000, lr: float = 0.01,
                 weight_decay: float = 0.0, test_interval: int = 20, select: str = "scripts", weight: Optional[Tensor] = None,
                 bias: Optional[Tensor] = None, generator=None, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8) -> dict:
    """R linear probes in one call on the device (rlap_linear_probe): LREvaluator's loop of the reference's scripts
    (scripts/node_shared.py:163-230; select="scripts") or CCA-SSG/main.py:152-194's (select="cca") -- full-batch Adam on a
    Linear(F, C) under log-softmax + NLL, scored on a validation and a test set, the selection rule applied on the device.

      x            : (N, F) float32, 1 <= F <= 512; detached, never differentiated.  A view with unit column stride is read in place.
      y            : (N,) int64 labels in [0, C); C = num_classes, or y.max() + 1 (the one host read before the call); 2 <= C <= 64
      train, valid, test : the rows of the R runs: an int64 index tensor (R = 1), a list of R index tensors (ragged), or a tuple
                     (indices, ptr) with ptr on the host.  Any order, a repeated row counts twice, sums run in list order; no set empty.
      weight, bias : (R, C, F), (R, C) float32 initial parameters; None draws them with `generator` as the reference does (probe_init)
      select       : "scripts": after every epoch e with (e + 1) % test_interval == 0, when val_micro > best_val_micro record the test
                     micro-F1, macro-F1, accuracy and e.  "cca": after every epoch, if val_acc >= best_val: best_val = val_acc, and if
                     test_acc > eval_acc: record.  Both compare integer counts of correct rows.
    Returns a dict of device tensors: micro_f1, macro_f1, accuracy (R,) float64; best_epoch, best_val_correct (R,) int64; weight, bias
    (the final parameters); loss (R,) float64, the last epoch's training loss; confusion (R, 2, C, C) int64, validation and test at the
    recorded evaluation, rows true, columns predicted; status, one int32: 0, or 2 / 3 when a kernel met an index outside [0, N) / a
    label outside [0, C) (reading it synchronises; adapters.LREvaluator does).  No host synchronisation inside the call.  Every
    value and the order of every sum are fixed (rlap_amd/csrc/rlap_probe.h): the same arguments give the same bits.
    """
    n, f, c = _probe_inputs(x, y, num_classes)
    lists = [_probe_lists(a, what) for a, what in ((train, "train"), (valid, "valid"), (test, "test"))]
    r = len(lists[0][1]) - 1
    if any(len(p) - 1 != r for _, p in lists):
        raise ValueError("train, valid, test: the same number of runs")
    if r > PROBE_MAX_RUNS:
        raise ValueError(f"at most {PROBE_MAX_RUNS} runs a call, got {r}")
    if select not in PROBE_SELECT:
        raise ValueError(f"select: one of {sorted(PROBE_SELECT)}, got {select!r}")
    epochs, test_interval = int(epochs), int(test_interval)
    if epochs < 1 or test_interval < 1:
        raise ValueError("epochs and test_interval: at least 1")
    lr, weight_decay, eps = float(lr), float(weight_decay), float(eps)
    b1, b2 = float(betas[0]), float(betas[1])
    if not (abs(lr) < float("inf")):
        raise ValueError(f"lr: finite, got {lr!r}")
    if not (0.0 <= weight_decay < float("inf")) or not (0.0 <= b1 < 1.0) or not (0.0 <= b2 < 1.0) or not (0.0 < eps < float("inf")):
        raise ValueError("weight_decay >= 0, betas in [0, 1), eps > 0")
    if (weight is None) != (bias is None):
        raise ValueError("weight and bias: both or neither")
    if weight is None:
        weight, bias = probe_init(r, c, f, generator)
    if not isinstance(weight, Tensor) or weight.dtype != torch.float32 or tuple(weight.shape) != (r, c, f):
        raise ValueError(f"weight: a ({r}, {c}, {f}) torch.float32 tensor")
    if not isinstance(bias, Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (r, c):
        raise ValueError(f"bias: a ({r}, {c}) torch.float32 tensor")
    dev = _device_for(x)
    with torch.cuda.device(dev):
        d_x, ldx = _probe_x(x, dev)
        d_y = y.to(device=dev).contiguous()
        d_l = [flat.to(device=dev).contiguous() for flat, _ in lists]
        h_p = [_i64_array(p) for _, p in lists]
        w0 = weight.detach().to(device=dev).contiguous()
        b0 = bias.detach().to(device=dev).contiguous()
        w, b = torch.empty_like(w0), torch.empty_like(b0)
        scores = torch.empty((r, 4), dtype=torch.float64, device=dev)
        best = torch.empty((r, 2), dtype=torch.int64, device=dev)
        conf = torch.empty((r, 2, c, c), dtype=torch.int64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _device_call("rlap_linear_probe", _lib.ProbeInfo, dev, 1, (
            d_x.data_ptr(), n, f, ldx, d_y.data_ptr(), c, r, d_l[0].data_ptr(), h_p[0], d_l[1].data_ptr(), h_p[1], d_l[2].data_ptr(), h_p[2],
            epochs, lr, weight_decay, test_interval, PROBE_SELECT[select], b1, b2, eps, w0.data_ptr(), b0.data_ptr(), w.data_ptr(),
            b.data_ptr(), scores.data_ptr(), best.data_ptr(), conf.data_ptr(), status.data_ptr()))
    return {"micro_f1": scores[:, 0], "macro_f1": scores[:, 1], "accuracy": scores[:, 2], "loss": scores[:, 3], "best_epoch": best[:, 0],
            "best_val_correct": best[:, 1], "weight": w, "bias": b, "confusion": conf, "status": status}


def probe_scores(x: Tensor, y: Tensor, index, weight: Tensor, bias: Tensor) -> dict:
    """The scoring pass of linear_probe alone (rlap_probe_scores): the predictions of R probes on their index lists and sklearn's
    scores of them.  `index` has the forms of linear_probe's sets; weight (R, C, F) and bias (R, C) float32 (or (C, F), (C,) for one
    run); C is weight's.  Returns a dict of device tensors: pred (int64, one per listed row, the lowest index among the largest
    logits), confusion (R, C, C) int64 (rows true, columns predicted), micro_f1, macro_f1, accuracy (R,) float64, status.
    macro_f1 is the plain mean of 2 tp / (2 tp + fp + fn) over the labels that occur among the true or the predicted labels.
    No host synchronisation."""
    if isinstance(weight, Tensor) and weight.dim() == 2 and isinstance(bias, Tensor) and bias.dim() == 1:
        weight, bias = weight[None], bias[None]
    if not isinstance(weight, Tensor) or weight.dim() != 3 or weight.dtype != torch.float32:
        raise ValueError("weight: a (R, C, F) torch.float32 tensor")
    n, f, c = _probe_inputs(x, y, int(weight.shape[1]))
    flat, ptr = _probe_lists(index, "index")
    r = len(ptr) - 1
    if r > PROBE_MAX_RUNS:
        raise ValueError(f"at most {PROBE_MAX_RUNS} runs a call, got {r}")
    if tuple(weight.shape) != (r, c, f):
        raise ValueError(f"weight: a ({r}, {c}, {f}) torch.float32 tensor")
    if not isinstance(bias, Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (r, c):
        raise ValueError(f"bias: a ({r}, {c}) torch.float32 tensor")
    dev = _device_for(x)
    with torch.cuda.device(dev):
        d_x, ldx = _probe_x(x, dev)
        d_y = y.to(device=dev).contiguous()
        d_i = flat.to(device=dev).contiguous()
        h_p = _i64_array(ptr)
        d_w = weight.detach().to(device=dev).contiguous()
        d_b = bias.detach().to(device=dev).contiguous()
        pred = torch.empty(ptr[-1], dtype=torch.int64, device=dev)
        conf = torch.empty((r, c, c), dtype=torch.int64, device=dev)
        scores = torch.empty((r, 3), dtype=torch.float64, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _device_call("rlap_probe_scores", _lib.ProbeInfo, dev, 1, (
            d_x.data_ptr(), n, f, ldx, d_y.data_ptr(), c, r, d_i.data_ptr(), h_p, d_w.data_ptr(), d_b.data_ptr(), pred.data_ptr(), conf.data_ptr(),
            scores.data_ptr(), status.data_ptr()))
    return {"pred": pred, "confusion": conf, "micro_f1": scores[:, 0], "macro_f1": scores[:, 1], "accuracy": scores[:, 2], "status": status}


def _plan_call(plan, flags: int, d_x: Tensor, F: int, y: Tensor):
    """One rlap_snapshot_plan_propagate call on the plan's device: the arena is sized by the call itself (RLAP_E_WORKSPACE and one
    regrow), statuses become exceptions as in _snapshot_call, `last_stats` is set on success."""
    global last_stats
    dev = plan.buffer.device
    lib, hobj = _handle_obj(dev)
    info = _lib.SpmmInfo()
    st = _lib.Stats()
    rc = _run(hobj, dev, 0, None, 1, False, lambda: lib.rlap_snapshot_plan_propagate(
        hobj.ptr, plan.buffer.data_ptr(), ctypes.byref(plan.desc), flags, d_x.data_ptr() if d_x.numel() else None, F,
        y.data_ptr() if y.numel() else None, ctypes.byref(info)), st)
    if rc in (1, 2, 3, _lib.E_NOT_GROUPED):
        raise ValueError(f"rlap: {_lib.status_string(rc)}")
    if rc != 0:
        _raise(rc)
    last_stats = info.as_dict()
    return info


def _plan_propagate(plan, x: Tensor, per_layer: bool, transpose: bool) -> Tensor:
    """One planned product; x and the direction are already checked."""
    dev = plan.buffer.device
    flags = ((_lib.SPMM_TRANSPOSE if transpose else 0) | (_lib.SPMM_X_F32 if x.dtype == torch.float32 else 0)
             | (_lib.SPMM_X_PER_LAYER if per_layer else 0))
    with torch.cuda.device(dev):
        d_x = x.detach().to(device=dev).contiguous()
        F = int(d_x.shape[-1])
        y = torch.empty((plan.layers, plan.num_nodes, F), dtype=d_x.dtype, device=dev)
        _plan_call(plan, flags, d_x, F, y)
        return y


class _PlanPropagate(torch.autograd.Function):
    """_Propagate over a plan: the gradient with respect to x is the planned call with `transpose` flipped."""

    @staticmethod
    def forward(ctx, x, plan, per_layer, transpose):
        ctx.call = (plan, per_layer, transpose)
        return _plan_propagate(plan, x, per_layer, transpose)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        plan, per_layer, transpose = ctx.call
        gx = _plan_propagate(plan, gy.contiguous(), True, not transpose)
        return (gx if per_layer else gx.sum(0)), None, None, None


class SnapshotPlan:
    """What snapshot_plan returns: the lists of snapshot_propagate for one elimination result, built once.  `buffer` is the plan (a
    torch.uint8 tensor on the device, owned by this object; valid while it is unchanged, and independent of `sc` after the build),
    `desc` its host descriptor (rlap_plan_desc), `info` what the build did (rlap_plan_info).

      layers, num_nodes : the shape of a result, (layers, num_nodes, F)
      entries           : entries of the list the products run over (rows that stay + loops)
      nbytes            : bytes of the plan buffer
      directions        : "forward", "transposed" or "both"
    """

    def __init__(self, buffer: Tensor, desc, info: dict, directions: str):
        self.buffer, self.desc, self.info, self.directions = buffer, desc, info, directions
        self.layers = int(desc.segments) // int(desc.graphs)
        self.num_nodes = int(desc.num_nodes)
        self.entries = int(info["entries"])
        self.nbytes = int(buffer.numel())

    def _need(self, transpose: bool):
        if not PLAN_DIRECTIONS[self.directions] & (_lib.PLAN_TRANSPOSED if transpose else _lib.PLAN_FORWARD):
            raise ValueError(f"this plan holds the {self.directions} lists only: build it with directions=\"both\" for "
                             f"transpose={transpose} (the backward pass of a product needs the other direction)")

    def propagate(self, x: Tensor, transpose: bool = False) -> Tensor:
        """y[l] = A^_l x (transpose: its transposed product) as ops.snapshot_propagate returns it for the plan's input and flags --
        the same bits -- without the preparation and without a host synchronisation.  x is (num_nodes, F) or (layers, num_nodes, F),
        float32 or float64.  Differentiable in x; the backward pass is the planned call of the other direction, so a plan of one
        direction refuses an x that requires a gradient.  Sets `last_stats` (rlap_spmm_info; host_syncs is 0)."""
        per_layer = _features_arg(x, self.num_nodes, self.layers)
        transpose = bool(transpose)
        self._need(transpose)
        if torch.is_grad_enabled() and x.requires_grad:
            self._need(not transpose)
            return _PlanPropagate.apply(x, self, per_layer, transpose)
        return _plan_propagate(self, x, per_layer, transpose)


def snapshot_plan(
    sc: Tensor,
    ptr: Union[Tensor, Sequence[int]],
    num_nodes: int,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    weighted: bool = False,
    add_self_loops: bool = True,
    fill_value: float = 1.0,
    normalize: bool = True,
    directions: str = "both",
) -> SnapshotPlan:
    """The x-independent half of snapshot_propagate, built once: a `SnapshotPlan` whose `.propagate(x, transpose)` returns what
    snapshot_propagate(sc, ptr, num_nodes, x, node_ptr, weighted, add_self_loops, fill_value, normalize, transpose) returns -- the
    same bits, for every F, float32 and float64, shared and per-layer x -- without the table checks, the column pass, the degrees, the
    sort by source and the host synchronisation that every unplanned call repeats.  One training step makes six to twelve products on
    the same (sc, ptr): build the plan after the elimination and use it for all of them.  All arguments as for snapshot_propagate;

      directions : "forward", "transposed" or "both" (default) -- the lists to build.  The backward pass of a product is the other
                   direction, so training needs "both"; a plan of one direction is about half the size.

    The plan lives in a torch.uint8 tensor on sc's device (16 bytes per row and direction, 8 to 24 bytes per (layer, id)); `sc` may be
    freed or overwritten after the build.  Malformed arguments raise ValueError before the device is touched; layout errors and (with
    weighted and normalize) a weight that is not finite or <= 0 raise ValueError as for snapshot_gcn_norm.  One host synchronisation.
    `last_stats` then holds what the build did (rlap_plan_info: entries, blocks, chunked_lists_forward, chunked_lists_transposed,
    loops_removed, arena_bytes, host_syncs)."""
    return _plan_build("rlap_snapshot_plan_build", sc, ptr, num_nodes, node_ptr, weighted, add_self_loops, fill_value, normalize, directions)


def _plan_build(export: str, sc, ptr, num_nodes, node_ptr, weighted, add_self_loops, fill_value, normalize, directions,
                extra_msg: Optional[str] = None, range_msg: Optional[str] = None) -> SnapshotPlan:
    """What snapshot_plan and edge_list_plan share: the host checks, the size query, the buffer, the build `export`, the trimming."""
    p, np_ = _snapshot_tables(sc, ptr, num_nodes, node_ptr)
    fill = _real(fill_value, "fill_value", 0.0, float("inf"))
    if directions not in PLAN_DIRECTIONS:
        raise ValueError(f"directions: one of {sorted(PLAN_DIRECTIONS)}, got {directions!r}")
    S, G, n = p.numel() - 1, _graphs(np_), int(num_nodes)
    if S < 1 or S % G != 0:
        raise ValueError(f"ptr: {S} segments; at least one, and a multiple of the {G} graphs")
    dev = _device_for(sc)
    flags = ((_lib.GCN_WEIGHTED if weighted else 0) | (_lib.GCN_SELF_LOOPS if add_self_loops else 0)
             | (_lib.GCN_NORMALIZE if normalize else 0) | PLAN_DIRECTIONS[directions])
    with torch.cuda.device(dev):
        rows = sc.to(device=dev, dtype=torch.float64).contiguous()
        lib, _ = _handle_obj(dev)
        bound = ctypes.c_size_t(0)
        rc = lib.rlap_snapshot_plan_bytes(int(rows.shape[0]), S, G, n, flags, ctypes.byref(bound))
        if rc != 0:
            _raise(rc)
        buf = torch.empty(int(bound.value), dtype=torch.uint8, device=dev)
        desc = _lib.PlanDesc()
        try:
            info = _snapshot_call(export, _lib.PlanInfo, rows, p, np_, n, (flags, fill, buf.data_ptr(), buf.numel(), ctypes.byref(desc)),
                                  extra_msg=extra_msg)
        except ValueError as e:
            if range_msg and str(e) == f"rlap: {_lib.status_string(_lib.E_INDEX_RANGE)}":
                raise ValueError(str(e) + range_msg) from None
            raise
        used = int(desc.plan_bytes)
        if 0 < used < buf.numel():   # (an input with loop rows, or few long lists: the tail is not in use)
            buf = buf[:used].clone() if 4 * used < 3 * buf.numel() else buf[:used]
        return SnapshotPlan(buf, desc, info.as_dict(), directions)


def edge_list_plan(
    rows: Tensor,
    ptr: Union[Tensor, Sequence[int]],
    num_nodes: int,
    node_ptr: Optional[Union[Tensor, Sequence[int]]] = None,
    weighted: bool = False,
    add_self_loops: bool = True,
    fill_value: float = 1.0,
    normalize: bool = True,
    directions: str = "both",
) -> SnapshotPlan:
    """snapshot_plan for a row table in ANY order: the (out, pptr) of snapshot_ppr, a snapshot_subgraph result, any (m, 3) table
    [source, target, w] whose S segments (segment = layer * G + graph) hold their rows in whatever order.  Duplicate rows, directed
    structure, loop rows and ids without rows are legal; nothing is coalesced.  The arguments are snapshot_plan's and so is the
    result: a `SnapshotPlan` whose `.propagate`, autograd and SnapshotGCNConv work unchanged.

    What the plan holds depends on a row's place in the input alone (rlap_amd/csrc/rlap_edgeplan.h): the list of target j is the
    rows with target j in input order, the transposed list of source i the rows with source i in input order; deg[j] is summed over
    j's list in the fixed order of snapshot_gcn_norm, the loop's weight (that of j's last loop row, or fill_value) last; an id
    without incoming rows has the loop's weight alone, or degree 0 (coefficient 0) without loops.  For an input in the elimination
    layout the buffer equals snapshot_plan's bit for bit.  The same input gives the same bits.

    Malformed arguments raise ValueError before the device is touched; an id that is not an integer of its graph's range and (with
    weighted and normalize) a weight that is not finite or <= 0 raise ValueError and say which.  One host synchronisation; `last_stats`
    holds rlap_plan_info (`blocks`: the non-empty forward lists)."""
    return _plan_build("rlap_edge_plan_build", rows, ptr, num_nodes, node_ptr, weighted, add_self_loops, fill_value, normalize, directions,
                       extra_msg=" (with weighted and normalize: a weight is not finite or <= 0)",
                       range_msg=" (an id of the rows is not an integer of its graph's range)")


def edge_plan(
    edge_index: Tensor,
    edge_weight: Optional[Tensor] = None,
    num_nodes: Optional[int] = None,
    add_self_loops: bool = True,
    fill_value: float = 1.0,
    normalize: bool = True,
    directions: str = "both",
) -> SnapshotPlan:
    """The plan of a plain graph: `edge_index` (2, E) integer, source row 0 and target row 1 (flow="source_to_target"), in any
    order; one segment, one layer; weighted iff `edge_weight` (E,) is given; `num_nodes=None` means edge_index.max() + 1.  A PyG
    batch is one block-diagonal graph.  plan.propagate(x)[0] is then GCNConv's A^ x of the graph itself, with the normalisation,
    the summation order and the bits of the snapshots' plans -- see edge_list_plan.  The rows are formed in torch: a plan is built
    once per graph."""
    if not isinstance(edge_index, Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index: a (2, E) integer tensor")
    if edge_index.dtype.is_floating_point or edge_index.dtype.is_complex or edge_index.dtype == torch.bool:
        raise ValueError(f"edge_index: an integer tensor, got {edge_index.dtype}")
    E = int(edge_index.shape[1])
    if edge_weight is not None:
        if not isinstance(edge_weight, Tensor) or edge_weight.dim() != 1 or edge_weight.shape[0] != E:
            raise ValueError(f"edge_weight: a ({E},) tensor, one weight per column of edge_index")
        if not edge_weight.dtype.is_floating_point:
            raise ValueError(f"edge_weight: a floating-point tensor, got {edge_weight.dtype}")
    if num_nodes is not None:
        n = _num_nodes(num_nodes)
    fill = _real(fill_value, "fill_value", 0.0, float("inf"))
    if directions not in PLAN_DIRECTIONS:
        raise ValueError(f"directions: one of {sorted(PLAN_DIRECTIONS)}, got {directions!r}")
    dev = _device_for(edge_index)
    with torch.cuda.device(dev):
        ei = edge_index.to(dev)
        if num_nodes is None:
            n = int(ei.max().item()) + 1 if E else 0
        rows = torch.empty((E, 3), dtype=torch.float64, device=dev)
        rows[:, 0], rows[:, 1] = ei[0], ei[1]
        rows[:, 2] = edge_weight.detach().to(dev) if edge_weight is not None else 1.0
    return edge_list_plan(rows, [0, E], n, None, edge_weight is not None, add_self_loops, fill, normalize, directions)


def _feature_apply(plan, w: Tensor, keep: Optional[Tensor], views: int, transpose: bool) -> Tensor:
    """One rlap_feature_plan_apply call; the operands are already checked, on the plan's device and contiguous.  Forward: w is
    (Fin, Fout) and the result (views, N, Fout); transposed: w is G (views, N, Fout) and the result (Fin, Fout)."""
    dev = plan.buffer.device
    flags = (_lib.SPMM_TRANSPOSE if transpose else 0) | (_lib.SPMM_X_F32 if w.dtype == torch.float32 else 0)
    with torch.cuda.device(dev):
        fout = int(w.shape[-1])
        shape = (plan.in_features, fout) if transpose else (views, plan.num_nodes, fout)
        out = torch.empty(shape, dtype=w.dtype, device=dev)
        _device_call("rlap_feature_plan_apply", _lib.FeatureInfo, dev, 1, (
            plan.buffer.data_ptr(), ctypes.byref(plan.desc), flags, w.data_ptr(), keep.data_ptr() if keep is not None else None,
            views, fout, out.data_ptr()))
        return out


class _FeatureLinear(torch.autograd.Function):
    """(x * keep[k]) @ W over a feature plan; the gradient with respect to W is the plan's transposed call on the upstream gradient."""

    @staticmethod
    def forward(ctx, weight, plan, keep, views):
        ctx.call = (plan, keep, views)
        return _feature_apply(plan, weight.detach().contiguous(), keep, views, False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        plan, keep, views = ctx.call
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        if not PLAN_DIRECTIONS[plan.directions] & _lib.PLAN_TRANSPOSED:
            raise RuntimeError(f"this feature plan holds the {plan.directions} lists only: the gradient with respect to weight is the "
                               "transposed call; build the plan with directions=\"both\"")
        return _feature_apply(plan, gy.contiguous(), keep, views, True), None, None, None


class FeaturePlan:
    """What feature_plan returns: the non-zeros of a dense (N, Fin) feature matrix as lists, built once.  `buffer` is the plan (a
    torch.uint8 tensor on the device, owned by this object and independent of x after the build), `desc` its host descriptor
    (rlap_feature_desc), `info` what the build did (rlap_feature_info: nnz, longest_forward / _transposed, long_lists_*, chunks_*,
    arena_bytes, host_syncs).

      num_nodes, in_features : N and Fin
      nnz                    : kept entries
      directions             : "forward", "transposed" or "both"
      nbytes                 : bytes of the plan buffer
    """

    def __init__(self, buffer: Tensor, desc, info: dict, directions: str):
        self.buffer, self.desc, self.info, self.directions = buffer, desc, info, directions
        self.num_nodes, self.in_features, self.nnz = int(desc.num_nodes), int(desc.in_features), int(desc.nnz)
        self.nbytes = int(buffer.numel())

    def linear(self, weight: Tensor, keep: Optional[Tensor] = None) -> Tensor:
        """(x * keep[k]) @ weight for every view k, without the masked copies of x: (K, N, Fout) for a (K, Fin) bool / uint8 `keep`
        (non-zero = the view keeps the column; K <= 32), or x @ weight as (N, Fout) for keep=None.  `weight` is (Fin, Fout), float32
        or float64, on the plan's device.  float64 sums in the fixed order of rlap_amd/csrc/rlap_featlin.h, rounded once: the same
        bits on every run.  Differentiable in `weight` alone; the backward pass is the plan's transposed call
        dW = sum_k keep[k][:, None] * (x^T G[k]), so a plan without the transposed direction raises there.  No host
        synchronisation.  Sets `last_stats` (rlap_feature_info)."""
        if not isinstance(weight, Tensor) or weight.dim() != 2 or weight.shape[0] != self.in_features or weight.shape[1] < 1:
            raise ValueError(f"weight: an ({self.in_features}, Fout) tensor, Fout >= 1")
        if weight.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"weight: float32 or float64, got {weight.dtype}")
        if weight.device != self.buffer.device:
            raise ValueError(f"weight: on the plan's device {self.buffer.device}, got {weight.device}")
        views = 1
        if keep is not None:
            if not isinstance(keep, Tensor) or keep.dim() != 2 or keep.shape[1] != self.in_features or keep.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"keep: None or a (K, {self.in_features}) bool or uint8 tensor")
            views = int(keep.shape[0])
            if not 1 <= views <= _lib.FEAT_MAX_VIEWS:
                raise ValueError(f"keep: 1 to {_lib.FEAT_MAX_VIEWS} views, got {views}")
        if not PLAN_DIRECTIONS[self.directions] & _lib.PLAN_FORWARD:
            raise ValueError("this feature plan holds the transposed lists only: build it with directions=\"forward\" or \"both\"")
        d_keep = keep.detach().to(device=self.buffer.device, dtype=torch.uint8).contiguous() if keep is not None else None
        if torch.is_grad_enabled() and weight.requires_grad:
            y = _FeatureLinear.apply(weight, self, d_keep, views)
        else:
            y = _feature_apply(self, weight.detach().contiguous(), d_keep, views, False)
        return y if keep is not None else y[0]


def feature_plan(x: Tensor, directions: str = "both") -> FeaturePlan:
    """The sparse first layer's plan: the entries of the dense (N, Fin) float32 or float64 matrix `x` with (double)x != 0.0 (-0.0 is
    dropped, NaN and infinities stay) as lists by row and by column, built once per run -- bag-of-words features are the same in
    every step.  `.linear(weight, keep)` then gives every view's (x * keep[k]) @ weight from one pass over a row's list, and its
    backward pass dW; the dense masked copies of adapters.drop_feature never exist.  `x` must not require a gradient (the call is
    differentiable in the weight alone).

      directions : "forward", "transposed" or "both" (default) -- the lists to build; training needs "both".

    The plan lives in a torch.uint8 tensor on x's device (16 bytes per non-zero and direction); x may be freed after the build.
    Malformed arguments raise ValueError before the device is touched.  Two host synchronisations (the count, then the build).
    `last_stats` then holds rlap_feature_info."""
    if not isinstance(x, Tensor) or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("x: a dense (N, Fin) tensor, N >= 1 and Fin >= 1")
    if x.layout != torch.strided or x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"x: a dense float32 or float64 tensor, got {x.dtype} ({x.layout})")
    if x.requires_grad:
        raise ValueError("x: must not require a gradient (FeaturePlan.linear is differentiable in the weight alone)")
    if directions not in PLAN_DIRECTIONS:
        raise ValueError(f"directions: one of {sorted(PLAN_DIRECTIONS)}, got {directions!r}")
    N, Fin = int(x.shape[0]), int(x.shape[1])
    dev = _device_for(x)
    flags = (_lib.FEAT_X_F32 if x.dtype == torch.float32 else 0) | PLAN_DIRECTIONS[directions]
    with torch.cuda.device(dev):
        d_x = x.detach().to(device=dev).contiguous()
        lib, hobj = _handle_obj(dev)
        nnz = ctypes.c_int64(0)
        rc = _run(hobj, dev, 0, None, 1, False, lambda: lib.rlap_feature_count(
            hobj.ptr, d_x.data_ptr(), N, Fin, flags & _lib.FEAT_X_F32, ctypes.byref(nnz)), _lib.Stats())
        if rc != 0:
            _raise(rc)
        bound = ctypes.c_size_t(0)
        rc = lib.rlap_feature_plan_bytes(N, Fin, int(nnz.value), flags, ctypes.byref(bound))
        if rc != 0:
            _raise(rc)
        buf = torch.empty(int(bound.value), dtype=torch.uint8, device=dev)
        desc = _lib.FeatureDesc()
        info = _device_call("rlap_feature_plan_build", _lib.FeatureInfo, dev, 1, (
            d_x.data_ptr(), N, Fin, int(nnz.value), flags, buf.data_ptr(), buf.numel(), ctypes.byref(desc)))
        return FeaturePlan(buf, desc, info.as_dict(), directions)


def feature_masks(in_features: int, p: float, views: int = 1, generator=None, device=None) -> Tensor:
    """The keep masks of FeaturePlan.linear, (views, in_features) bool, drawn as adapters.drop_feature draws its drop masks: per view
    `torch.empty(in_features).uniform_(0, 1, generator=generator) < p` is dropped.  Under equally seeded generators on the same
    device, x * keep[k] equals drop_feature(x, p, views, generator)[k].  `device` defaults to the generator's, else the CPU."""
    fin = _count(in_features, "in_features", 1, 2**31 - 1)
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"p: in [0, 1], got {p!r}")
    k = _count(views, "views", 1, _lib.FEAT_MAX_VIEWS)
    if device is None:
        device = generator.device if generator is not None else torch.device("cpu")
    keep = torch.empty((k, fin), dtype=torch.bool, device=device)
    for v in range(k):
        keep[v] = ~(torch.empty((fin,), dtype=torch.float32, device=device).uniform_(0, 1, generator=generator) < p)
    return keep


DROP_AGGR = {"sink": 0, "source": _lib.DROP_SOURCE}
DROP_MAX_STEPS = 100000   # cap on pr_iters and evc_max_iter (rlap_amd/csrc/rlap_edgedrop.h)


def _count(x, what: str, lo: int, hi: int) -> int:
    if isinstance(x, bool) or not hasattr(x, "__index__") or not lo <= x.__index__() <= hi:
        raise ValueError(f"{what}: an integer in [{lo}, {hi}], got {x!r}")
    return x.__index__()


def _unit(x, what: str) -> float:
    """A number in [0, 1]: anything with __float__ that is no bool or string (Python and numpy scalars, 0-d tensors)."""
    try:
        v = None if isinstance(x, (bool, str, bytes)) or not hasattr(x, "__float__") else float(x)
    except (TypeError, ValueError, RuntimeError):
        v = None
    if v is None or not 0.0 <= v <= 1.0:
        raise ValueError(f"{what}: a number in [0, 1], got {x!r}")
    return v


def _drop_ps(p) -> list:
    """The K values of `p`: one number, or any sequence of them (list, tuple, ndarray, 1-D tensor)."""
    if isinstance(p, (str, bytes)) or getattr(p, "ndim", 1) == 0 or not hasattr(p, "__iter__"):
        ps = [p]
    else:
        ps = list(p.tolist() if hasattr(p, "tolist") else p)
    if not 1 <= len(ps) <= _lib.DROP_MAX_VIEWS:
        raise ValueError(f"p: one number or a sequence of 1 to {_lib.DROP_MAX_VIEWS} numbers, got {len(ps)}")
    return [_unit(v, "p") for v in ps]


def _drop_args(edge_index, edge_weight, num_nodes, p, scheme, threshold, seed, aggr, pr_damp, pr_iters, evc_tol, evc_max_iter):
    """Host-side checks of drop_edges, made before anything is launched: (E, n or None, the K values of p, the export's scalars)."""
    if not isinstance(edge_index, Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index: a (2, E) integer tensor")
    if edge_index.dtype.is_floating_point or edge_index.dtype.is_complex or edge_index.dtype == torch.bool:
        raise ValueError(f"edge_index: an integer tensor, got {edge_index.dtype}")
    E = int(edge_index.shape[1])
    if edge_weight is not None:
        if not isinstance(edge_weight, Tensor) or edge_weight.dim() != 1 or edge_weight.shape[0] != E:
            raise ValueError(f"edge_weight: a ({E},) tensor, one weight per column of edge_index")
        if not edge_weight.dtype.is_floating_point:
            raise ValueError(f"edge_weight: a floating-point tensor, got {edge_weight.dtype}")
    n = None if num_nodes is None else _num_nodes(num_nodes)
    ps = _drop_ps(p)
    if scheme not in _lib.DROP_SCHEMES:
        raise ValueError(f"scheme: one of {sorted(_lib.DROP_SCHEMES)}, got {scheme!r}")
    if aggr not in DROP_AGGR:
        raise ValueError(f"aggr: one of {sorted(DROP_AGGR)}, got {aggr!r} (aggr='mean' needs a per-edge maximum and is not provided)")
    if seed is not None and (isinstance(seed, bool) or not hasattr(seed, "__index__")):
        raise ValueError(f"seed: an integer or None, got {seed!r}")
    if isinstance(evc_tol, bool) or not isinstance(evc_tol, (int, float)) or not 0.0 <= float(evc_tol) < float("inf"):
        raise ValueError(f"evc_tol: a finite number >= 0, got {evc_tol!r}")
    scalars = (_unit(threshold, "threshold"), _seed_from(None if seed is None else seed.__index__()), _unit(pr_damp, "pr_damp"),
               _count(pr_iters, "pr_iters", 0, DROP_MAX_STEPS), float(evc_tol), _count(evc_max_iter, "evc_max_iter", 1, DROP_MAX_STEPS))
    return E, n, ps, scalars


def drop_edges(
    edge_index: Tensor,
    edge_weight: Optional[Tensor] = None,
    num_nodes: Optional[int] = None,
    p=0.5,
    scheme: str = "uniform",
    threshold: float = 0.7,
    seed: Optional[int] = 0,
    aggr: str = "sink",
    pr_damp: float = 0.85,
    pr_iters: int = 10,
    evc_tol: float = 1e-6,
    evc_max_iter: int = 1000,
    return_mask: bool = False,
    return_scores: bool = False,
):
    """Centrality-adaptive edge dropping on the device, K views a call: EdgeDropping, EdgeDroppingDegree, EdgeDroppingPR and
    EdgeDroppingEVC of scripts/augmentor_benchmarks.py:216-363 (GCA's adaptive schemes) -- `scheme` "uniform", "degree", "pagerank",
    "eigenvector".  `edge_index` is (2, E), source row 0 and target row 1, in any order; duplicates, loops and directed edges stay as
    they are; a batch of graphs is its disjoint union.  `edge_weight` (E,) is carried to the output and never read for the scores.
    `num_nodes=None` means edge_index.max() + 1 (one torch reduction and read-back in front of the call).  `p` is one number or a
    sequence of K <= 32 numbers in [0, 1]: view k uses p[k] and seed + k, and equals a one-view call with those, bit for bit.
    `seed=None` draws a seed from torch's RNG (the adapters' default); with an integer the call is a pure function of its arguments.  `aggr`: a row's score is that of its target ("sink", the
    reference's choice) or of its source ("source").

    The centrality c is found once for all views: the degree after to_undirected; compute_pr's `pr_iters` steps with `pr_damp`; the
    power iteration of networkx's eigenvector_centrality on the multigraph of the rows (duplicates count), stopped after the step
    with sum |x' - x| <= N evc_tol or after `evc_max_iter` steps, then max(x, 0) + 1e-8.  With s = log c, taken over the rows:
    node_weight = ((smax - s) / (smax - smean)) / their mean; row e is dropped in view k with probability
    q = min(node_weight[endpoint] p[k], threshold) -- a NaN gives threshold -- and kept iff u(k, e) >= q, u a counter-based uniform
    of (seed + k, e).  Every rule and the order of every sum: rlap_amd/csrc/rlap_edgedrop.h.  All float64.

    Returns (rows, ptr): rows (M, 3) float64 [source, target, weight] (weight 1.0 without edge_weight), view-major, input order
    inside a view; ptr (K+1,) int64; both on the device -- what edge_list_plan takes.  With return_mask a (K, E) bool tensor follows,
    with return_scores a dict: centrality (N,), node_weight (N,) (zeros for "uniform"), iters, converged.  The same input gives
    the same bits.  Malformed arguments raise ValueError before the device is touched; an id outside [0, num_nodes) raises
    ValueError.  One host synchronisation inside the C call (num_nodes=None adds the read-back above); `last_stats` holds
    rlap_edge_drop_info."""
    E, n, ps, scalars = _drop_args(edge_index, edge_weight, num_nodes, p, scheme, threshold, seed, aggr, pr_damp, pr_iters, evc_tol, evc_max_iter)
    K = len(ps)
    dev = _device_for(edge_index)
    with torch.cuda.device(dev):
        ei = edge_index.to(device=dev, dtype=torch.int64)
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        w = edge_weight.detach().to(device=dev, dtype=torch.float64).contiguous() if edge_weight is not None else None
        if n is None:
            n = int(ei.max().item()) + 1 if E else 0
        cap = K * E
        rows = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        ptr = torch.empty(K + 1, dtype=torch.int64, device=dev)
        mask = torch.empty((K, E), dtype=torch.bool, device=dev) if return_mask else None
        cen = torch.empty(n, dtype=torch.float64, device=dev) if return_scores else None
        nw = torch.empty(n, dtype=torch.float64, device=dev) if return_scores else None
        threshold, seed, pr_damp, pr_iters, evc_tol, evc_max_iter = scalars
        info = _device_call("rlap_edge_drop", _lib.EdgeDropInfo, dev, 1, (
            src.data_ptr() if E else None, dst.data_ptr() if E else None, w.data_ptr() if w is not None and E else None, E, n,
            _lib.DROP_SCHEMES[scheme], DROP_AGGR[aggr], (ctypes.c_double * K)(*ps), K, threshold, seed, pr_damp, pr_iters, evc_tol, evc_max_iter,
            rows.data_ptr() if cap else None, cap, ptr.data_ptr(), mask.data_ptr() if mask is not None and E else None,
            cen.data_ptr() if cen is not None and n else None, nw.data_ptr() if nw is not None and n else None))
        out = [_trim(rows, int(info.rows_needed)), ptr]
    if return_mask:
        out.append(mask)
    if return_scores:
        out.append({"centrality": cen, "node_weight": nw, "iters": int(info.iters), "converged": bool(info.converged)})
    return tuple(out)


def _sample_seeds(num_seeds) -> list:
    """The K values of `num_seeds`: one integer, or any sequence of them (list, tuple, ndarray, 1-D tensor)."""
    if isinstance(num_seeds, (str, bytes)) or getattr(num_seeds, "ndim", 1) == 0 or not hasattr(num_seeds, "__iter__"):
        ns = [num_seeds]
    else:
        ns = list(num_seeds.tolist() if hasattr(num_seeds, "tolist") else num_seeds)
    if not 1 <= len(ns) <= _lib.DROP_MAX_VIEWS:
        raise ValueError(f"num_seeds: one integer or a sequence of 1 to {_lib.DROP_MAX_VIEWS} integers, got {len(ns)}")
    return [_count(v, "num_seeds", 0, _lib.SAMPLE_MAX_SEEDS) for v in ns]


def _sample_args(edge_index, edge_weight, num_nodes, scheme, p, num_seeds, walk_length, seed, return_walks):
    """Host-side checks of sample_subgraphs, made before anything is launched: (E, n or None, ps, seeds, walk_length, seed)."""
    if not isinstance(edge_index, Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index: a (2, E) integer tensor")
    if edge_index.dtype.is_floating_point or edge_index.dtype.is_complex or edge_index.dtype == torch.bool:
        raise ValueError(f"edge_index: an integer tensor, got {edge_index.dtype}")
    E = int(edge_index.shape[1])
    if edge_weight is not None:
        if not isinstance(edge_weight, Tensor) or edge_weight.dim() != 1 or edge_weight.shape[0] != E:
            raise ValueError(f"edge_weight: a ({E},) tensor, one weight per column of edge_index")
        if not edge_weight.dtype.is_floating_point:
            raise ValueError(f"edge_weight: a floating-point tensor, got {edge_weight.dtype}")
    n = None if num_nodes is None else _num_nodes(num_nodes)
    if scheme not in _lib.SAMPLE_SCHEMES:
        raise ValueError(f"scheme: one of {sorted(_lib.SAMPLE_SCHEMES)}, got {scheme!r}")
    ps, seeds, length = None, None, 0
    if scheme == "drop":
        ps = _drop_ps(p)
        if return_walks:
            raise ValueError("return_walks: only scheme='walk' has walks")
    else:
        if num_seeds is None:
            raise ValueError("num_seeds: scheme='walk' needs one integer or a sequence of 1 to 32 integers, got None")
        seeds = _sample_seeds(num_seeds)
        length = _count(walk_length, "walk_length", 0, _lib.SAMPLE_MAX_WALK_LENGTH)
        if any(seeds) and (n == 0 or (n is None and E == 0)):
            raise ValueError("num_seeds: walkers need a node to start from, and num_nodes is 0")
    if seed is not None and (isinstance(seed, bool) or not hasattr(seed, "__index__")):
        raise ValueError(f"seed: an integer or None, got {seed!r}")
    return E, n, ps, seeds, length, _seed_from(None if seed is None else seed.__index__())


def sample_subgraphs(
    edge_index: Tensor,
    edge_weight: Optional[Tensor] = None,
    num_nodes: Optional[int] = None,
    scheme: str = "drop",
    p=0.5,
    num_seeds=None,
    walk_length: int = 10,
    seed: Optional[int] = 0,
    return_nodes: bool = False,
    return_walks: bool = False,
):
    """Node dropping and random-walk subgraph views on the device, K views a call: PyGCL's NodeDropping(pn) (`scheme` "drop") and
    RWSampling(num_seeds, walk_length) ("walk") as the training scripts use them.  `edge_index` is (2, E), source row 0 and target
    row 1, in any order; duplicates, loops and directed edges stay as they are; a batch of graphs is its disjoint union.
    `edge_weight` (E,) is carried to the output and never read otherwise.  `num_nodes=None` means edge_index.max() + 1 (one torch
    reduction and read-back in front of the call).  "drop" takes `p`, one number or a sequence of K <= 32 numbers in [0, 1] (and
    ignores num_seeds and walk_length); "walk" takes `num_seeds`, one integer or K <= 32 integers >= 0, and `walk_length` in
    [0, 1024] (and ignores p).  View k uses p[k] or num_seeds[k], and seed + k, and equals a one-view call with those, bit for
    bit.  `seed=None` draws a seed from torch's RNG (the adapters' default); with an integer the call is a pure function of its
    arguments.

    A view is a node set, and a row is kept iff its source and its target are both in it (PyG's subgraph with
    relabel_nodes=False: the ids stay).  drop: node v is in the set iff its coin u_node(seed + k, v) >= p[k], so p = 0 keeps every
    node and p = 1 none.  walk: num_seeds[k] walkers start at uniform nodes and take walk_length steps, each to the target of a
    uniformly chosen outgoing row of the node they stand on (duplicates and loops count; a node without outgoing rows keeps its
    walker); the set is every node a walker stood on.  Every rule: rlap_amd/csrc/rlap_nodesample.h.

    Returns (rows, ptr) as drop_edges does: rows (M, 3) float64 [source, target, weight] (weight 1.0 without edge_weight),
    view-major, input order inside a view; ptr (K+1,) int64; both on the device -- what edge_list_plan takes.  With return_nodes a
    (K, N) bool tensor follows, the node sets; with return_walks (walk only) a (sum of num_seeds, walk_length + 1) int64 tensor, the
    walks, view-major.  The same input gives the same bits.  Malformed arguments, walkers without a node among them, raise ValueError
    before the device is touched; an id outside [0, num_nodes) raises ValueError.  One host synchronisation inside the C call
    (num_nodes=None adds the read-back above); `last_stats` holds rlap_node_sample_info."""
    E, n, ps, seeds, length, seed = _sample_args(edge_index, edge_weight, num_nodes, scheme, p, num_seeds, walk_length, seed, return_walks)
    K = len(ps if ps is not None else seeds)
    dev = _device_for(edge_index)
    with torch.cuda.device(dev):
        ei = edge_index.to(device=dev, dtype=torch.int64)
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        w = edge_weight.detach().to(device=dev, dtype=torch.float64).contiguous() if edge_weight is not None else None
        if n is None:
            n = int(ei.max().item()) + 1 if E else 0
        cap = K * E
        rows = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        ptr = torch.empty(K + 1, dtype=torch.int64, device=dev)
        nodes = torch.empty((K, n), dtype=torch.bool, device=dev) if return_nodes else None
        walkers = sum(seeds) if seeds is not None else 0
        walks = torch.empty((walkers, length + 1), dtype=torch.int64, device=dev) if return_walks else None
        info = _device_call("rlap_node_sample", _lib.NodeSampleInfo, dev, 1, (
            src.data_ptr() if E else None, dst.data_ptr() if E else None, w.data_ptr() if w is not None and E else None, E, n,
            _lib.SAMPLE_SCHEMES[scheme], (ctypes.c_double * K)(*ps) if ps is not None else None,
            (ctypes.c_int64 * K)(*seeds) if seeds is not None else None, K, length, seed,
            rows.data_ptr() if cap else None, cap, ptr.data_ptr(), nodes.data_ptr() if nodes is not None and n else None,
            walks.data_ptr() if walks is not None and walkers else None))
        out = [_trim(rows, int(info.rows_needed)), ptr]
    if return_nodes:
        out.append(nodes)
    if return_walks:
        out.append(walks)
    return tuple(out)


def _add_ratios(ratio) -> list:
    """The K values of `ratio`: one finite number >= 0, or any sequence of them (list, tuple, ndarray, 1-D tensor)."""
    if isinstance(ratio, (str, bytes)) or getattr(ratio, "ndim", 1) == 0 or not hasattr(ratio, "__iter__"):
        rs = [ratio]
    else:
        rs = list(ratio.tolist() if hasattr(ratio, "tolist") else ratio)
    if not 1 <= len(rs) <= _lib.DROP_MAX_VIEWS:
        raise ValueError(f"ratio: one number or a sequence of 1 to {_lib.DROP_MAX_VIEWS} numbers, got {len(rs)}")
    out = []
    for x in rs:
        try:
            v = None if isinstance(x, (bool, str, bytes)) or not hasattr(x, "__float__") else float(x)
        except (TypeError, ValueError, RuntimeError):
            v = None
        if v is None or not 0.0 <= v < float("inf"):
            raise ValueError(f"ratio: a finite number >= 0, got {x!r}")
        out.append(v)
    return out


def _add_args(edge_index, edge_weight, num_nodes, ratio, seed):
    """Host-side checks of add_edges, made before anything is launched: (E, n or None, the K counts int(E * ratio[k]), seed)."""
    if not isinstance(edge_index, Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index: a (2, E) integer tensor")
    if edge_index.dtype.is_floating_point or edge_index.dtype.is_complex or edge_index.dtype == torch.bool:
        raise ValueError(f"edge_index: an integer tensor, got {edge_index.dtype}")
    E = int(edge_index.shape[1])
    if edge_weight is not None:
        if not isinstance(edge_weight, Tensor) or edge_weight.dim() != 1 or edge_weight.shape[0] != E:
            raise ValueError(f"edge_weight: a ({E},) tensor, one weight per column of edge_index")
        if not edge_weight.dtype.is_floating_point:
            raise ValueError(f"edge_weight: a floating-point tensor, got {edge_weight.dtype}")
    n = None if num_nodes is None else _num_nodes(num_nodes)
    counts = [int(E * r) for r in _add_ratios(ratio)]      # the reference's expression, on Python floats
    if E + max(counts) > _lib.ADD_MAX_ROWS:
        raise ValueError(f"ratio: E + int(E * ratio) must stay below 2^31 - 1, got {E} + {max(counts)}")
    if any(counts) and n is not None and n < 2:
        raise ValueError(f"num_nodes: added edges draw their ends from [0, num_nodes - 2], which needs num_nodes >= 2, got {n}")
    if seed is not None and (isinstance(seed, bool) or not hasattr(seed, "__index__")):
        raise ValueError(f"seed: an integer or None, got {seed!r}")
    return E, n, counts, _seed_from(None if seed is None else seed.__index__())


def add_edges(
    edge_index: Tensor,
    edge_weight: Optional[Tensor] = None,
    num_nodes: Optional[int] = None,
    ratio=0.5,
    seed: Optional[int] = 0,
    coalesce: bool = True,
    return_added: bool = False,
):
    """Edge adding on the device, K views a call: the EdgeAdding augmentor of scripts/augmentor_benchmarks.py:44-65 (`coalesce=True`)
    and the add_edge of CCA-SSG/aug.py:95-104 (`coalesce=False`).  `edge_index` is (2, E), source row 0 and target row 1, in any
    order; duplicates, loops and directed edges are allowed; a batch of graphs is its disjoint union.  `num_nodes=None` means
    edge_index.max() + 1 (one torch reduction and read-back in front of the call).  `ratio` is one number or a sequence of K <= 32
    finite numbers >= 0 (values above 1 are allowed): view k adds int(E * ratio[k]) edges, uses seed + k, and equals a one-view call
    with those, bit for bit.  `seed=None` draws a seed from torch's RNG (the adapters' default); with an integer the call is a pure
    function of its arguments.

    Both ends of an added edge are uniform over [0, num_nodes - 2]: the reference draws torch.randint(0, num_nodes - 1, ...), whose
    upper end is exclusive, so the last node never receives an added edge -- restated as it stands.  Added edges may be loops, may
    repeat each other and may repeat input edges.  This is the reference's distribution, not torch's random stream.

    coalesce=True: view k holds the distinct (source, target) pairs of the input and the added edges, ascending by (source, target),
    the order of sort_edge_index and coalesce.  The weight of a pair is s_in + c_add: s_in the float64 sum of its input edges in
    input order (`edge_weight`, or 1.0 each; 0.0 without one), c_add the number of its added edges -- without edge_weight the
    multiplicity, which the reference computes and throws away.  The input is sorted at most once a call, whatever K is, and not at
    all when it is sorted already (a coalesced PyG graph is): `last_stats` reports input_sorted, sorts and launches.
    coalesce=False: view k is the E input edges in input order, then its added edges in draw order with weight 1.0.

    Returns (rows, ptr): rows (M, 3) float64 [source, target, weight], view-major; ptr (K+1,) int64; both on the device -- what
    edge_list_plan takes.  With return_added (added, aptr) follow: added (sum of the counts, 2) int64, the added pairs in draw order,
    view-major; aptr (K+1,) int64.  The same input gives the same bits.  Malformed arguments, num_nodes < 2 with an edge to add
    among them, raise ValueError before the call; an id outside [0, num_nodes) raises ValueError.  One host synchronisation inside
    the C call (num_nodes=None adds the read-back above): for an unsorted input it holds the row total all the same, and the sort
    and the rows follow on the stream; `last_stats` holds rlap_edge_add_info.  Every rule: rlap_amd/csrc/rlap_edgeadd.h."""
    E, n, counts, seed = _add_args(edge_index, edge_weight, num_nodes, ratio, seed)
    K, total_add = len(counts), sum(counts)
    dev = _device_for(edge_index)
    with torch.cuda.device(dev):
        ei = edge_index.to(device=dev, dtype=torch.int64)
        src, dst = ei[0].contiguous(), ei[1].contiguous()
        w = edge_weight.detach().to(device=dev, dtype=torch.float64).contiguous() if edge_weight is not None else None
        if n is None:
            n = int(ei.max().item()) + 1 if E else 0
            if total_add and n < 2:
                raise ValueError(f"num_nodes: added edges draw their ends from [0, num_nodes - 2], which needs num_nodes >= 2, got {n}")
        cap = K * E + total_add
        rows = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        ptr = torch.empty(K + 1, dtype=torch.int64, device=dev)
        added = torch.empty((total_add, 2), dtype=torch.int64, device=dev) if return_added else None
        aptr = torch.empty(K + 1, dtype=torch.int64, device=dev) if return_added else None
        info = _device_call("rlap_edge_add", _lib.EdgeAddInfo, dev, 1, (
            src.data_ptr() if E else None, dst.data_ptr() if E else None, w.data_ptr() if w is not None and E else None, E, n,
            (ctypes.c_int64 * K)(*counts), K, seed, _lib.ADD_COALESCE if coalesce else 0, rows.data_ptr() if cap else None, cap, ptr.data_ptr(),
            added.data_ptr() if added is not None else None, aptr.data_ptr() if aptr is not None else None))
        out = [_trim(rows, int(info.rows_needed)), ptr]
    if return_added:
        out += [added, aptr]
    return tuple(out)


def identity(a: Tensor) -> Tensor:
    """Boundary self-test (reference: rlap/ops.py:61-63): tensor -> column-major
    staging -> tensor, on the GPU; returns a tensor on `a`'s device."""
    assert a.dim() == 2
    dev = _device_for(a)
    lib, h = _handle(dev)
    with torch.cuda.device(dev):
        x = a.to(device=dev, dtype=torch.float64).contiguous()
        tmp = torch.empty_like(x)
        out = torch.empty_like(x)
        rc = lib.rlap_identity(h, x.data_ptr(), tmp.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1])
        if rc != 0:
            _raise(rc)
    return out.to(a.device)


def rng_uniforms(count: int, device=None) -> Tensor:
    """First `count` uniforms of the sampling stream as generated on the device."""
    dev = _device_for(None) if device is None else torch.device(device)
    lib, hobj = _handle_obj(dev)
    with torch.cuda.device(dev):
        out = torch.empty(count, dtype=torch.float64, device=dev)
        hobj.fit(dev, 0, max(int(count), 1 << 16))
        rc = lib.rlap_rng_uniforms(hobj.ptr, count, out.data_ptr())
        if rc != 0:
            _raise(rc)
    return out


# ---------------------------------------------------------------------------
# torch.ops.extension_cpp.* -- the reference's dispatcher-level interface
# (py_api_binder.cc:80-88), so third-party code calling the torch op still works.
# ---------------------------------------------------------------------------
def _op_approximate_cholesky(edge_info: Tensor, num_nodes: int, num_remove: int, o_v: str, o_n: str) -> Tensor:
    ei = edge_info
    edge_index = ei[:, :2].t().to(torch.int64)
    res = approximate_cholesky(edge_index, ei[:, 2], num_nodes, num_remove, o_v, o_n,
                               return_device="cpu" if not ei.is_cuda else "same")
    return res


def _op_identity(a: Tensor) -> Tensor:
    return identity(a)


def _register_torch_ops():
    try:
        lib = torch.library.Library("extension_cpp", "DEF")
        lib.define("approximate_cholesky(Tensor edge_info, int num_nodes, int num_remove, str o_v,  str o_n) -> Tensor")
        lib.define("identity(Tensor a) -> Tensor")
    except RuntimeError:
        return None  # namespace already defined (e.g. the reference extension is loaded too)
    for key in ("CPU", "CUDA"):
        lib.impl("approximate_cholesky", _op_approximate_cholesky, key)
        lib.impl("identity", _op_identity, key)
    return lib


_torch_lib = _register_torch_ops()
