"""Markov diffusion on the device (ops.snapshot_markov, rlap_markov.hip) regime by regime, against the host mirror bit for
bit (tests/test_gpu_markov.py says what the yardstick is):

  a. segments of 1, 2, 63, 64, 65, 128 and 129 nodes (one, two and three tiles), a hub row of 127 entries and hubs of 4 to 7
     entries (both sides of the four-in-flight loop), in one call and alone;
  b. 4,096 nodes (the last size of the one-workgroup regime) and 4,097 (the first of the launch-per-sweep regime): a weighted path
     with a few chords, so that the output stays a band, at orders 3 and 16;
  c. orders 1, 2, 3, 16 (both parities of the final copy), alpha 0 and 1, unit weights, no self loop, ids without edges and
     normalize_out in a call whose segments fall into both regimes;
  d. 65,537 two-node segments: a second group by the tile count, the output offset carried across;
  e. the output retry of the Python layer.
`last_stats` must show the regime every case is meant to reach (small / large tiles, groups, launches).  (A third regime with the
tiles in LDS for segments up to 128 nodes was measured and left out; the sizes around 128 stay as tile edges.)"""
import numpy as np
import pytest
import torch

import markov_mirror as mm
from test_gpu_markov import equals_mirror, graph_rows, markov_twice, same_bits
from util import path, star

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mm.build(tmp_path_factory.mktemp("markov"))


def weighted(ei, seed):
    ei = np.asarray(ei)
    return mm.column_layout(ei, mm.symmetric_weights(ei, seed))


def call_of(parts):
    sc = torch.from_numpy(np.concatenate(parts)).cuda()
    return sc, np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).tolist()


# ------------------------------------------------------------------------------------------------ a. tile edges
def edge_parts():
    loop = np.array([[5.0, 5.0, 1.5]])                                            # one node, one loop row
    return [loop, weighted(path(2), 1), weighted(path(63), 2), graph_rows(64, 3), graph_rows(65, 4), weighted(path(128), 5),
            graph_rows(129, 6), weighted(star(128), 7), weighted(star(5), 8), weighted(star(6), 9), weighted(star(7), 10),
            weighted(star(8), 11), graph_rows(128, 12, m=4)]


EDGE_NODES = [1, 2, 63, 64, 65, 128, 129, 128, 5, 6, 7, 8, 128]


@pytest.mark.parametrize("order", [16, 3])
def test_tile_edges_alone_and_together(ops, lib, order):
    parts = edge_parts()
    assert [len(np.unique(p[:, :2])) for p in parts] == EDGE_NODES
    assert [int((p[:, 1] == 0).sum()) for p in parts[7:12]] == [127, 4, 5, 6, 7]    # 31 * 4 + 3 and every remainder of the 4-way gather
    sc, ptr = call_of(parts)
    kw = dict(order=order, eps=1e-3)
    out, mptr, st = markov_twice(ops, sc, ptr, 200, **kw)
    assert (st["small_tiles"], st["large_tiles"], st["groups"]) == (sum(-(-n // 64) for n in EDGE_NODES), 0, 1)
    assert st["launches"] == 2 + 4                                                  # init and sweeps; 4 to keep
    equals_mirror(lib, out, mptr, parts, **kw)
    mp = mptr.tolist()
    for s, p in enumerate(parts):
        one = torch.from_numpy(p).cuda()
        alone, ap, st1 = markov_twice(ops, one, [0, p.shape[0]], 200, **kw)
        assert (st1["small_tiles"], st1["large_tiles"]) == (-(-EDGE_NODES[s] // 64), 0), s
        assert same_bits(out[mp[s]:mp[s + 1]], alone) and ap.tolist() == [0, mp[s + 1] - mp[s]], s
    norm, nptr, _ = markov_twice(ops, sc, ptr, 200, normalize_out=True, **kw)
    equals_mirror(lib, norm, nptr, parts, normalize=True, **kw)


# ------------------------------------------------------------------------------------------------ b. the regime edge
def band(n, seed):
    """A weighted path of n nodes with a chord i -- i + 3 at every 97th node: the diffusion stays a band."""
    i = np.arange(0, n - 3, 97)
    ei = np.concatenate([np.asarray(path(n)), np.stack([i, i + 3]), np.stack([i + 3, i])], 1)
    return weighted(ei, seed)


@pytest.fixture(scope="module")
def bands():
    return {4096: band(4096, 1), 4097: band(4097, 2)}


@pytest.mark.parametrize("order", [3, 16])
def test_regime_edge(ops, lib, bands, order):
    parts = [bands[4096], bands[4097]]
    sc, ptr = call_of(parts)
    kw = dict(order=order, eps=1e-4)
    out, mptr, st = markov_twice(ops, sc, ptr, 4097, **kw)
    assert (st["small_tiles"], st["large_tiles"], st["groups"]) == (64, 65, 2)
    assert st["launches"] == (2 + 4) + (1 + order + 1 + 4)                           # large: init, D + 1 sweeps, 4 to keep
    assert out.shape[0] < 4097 * 80                                                 # a band
    equals_mirror(lib, out, mptr, parts, **kw)
    mp = mptr.tolist()
    for s, (n, small, large) in enumerate([(4096, 64, 0), (4097, 0, 65)]):
        one = torch.from_numpy(parts[s]).cuda()
        alone, ap, st1 = markov_twice(ops, one, [0, one.shape[0]], 4097, **kw)
        assert (st1["small_tiles"], st1["large_tiles"], st1["groups"]) == (small, large, 1)
        assert same_bits(out[mp[s]:mp[s + 1]], alone) and ap.tolist() == [0, mp[s + 1] - mp[s]]
        i, j, v = alone[:, 0].long(), alone[:, 1].long(), alone[:, 2]
        kf, of = torch.sort(i * n + j)
        kb, ob = torch.sort(j * n + i)
        assert torch.equal(kf, kb) and same_bits(v[of], v[ob])                     # exactly symmetric


# ------------------------------------------------------------------------------------------------ c. both regimes at once
@pytest.fixture(scope="module")
def mixed(bands):
    """Segments of 50, 100, 200, 300 (small) and 4,097 (large) nodes."""
    return [graph_rows(50, 1), graph_rows(300, 2), bands[4097], graph_rows(100, 3), graph_rows(200, 4)]


MIXED = [dict(order=1), dict(order=2), dict(order=3), dict(order=16), dict(alpha=0.0, order=3), dict(alpha=1.0, order=2),
         dict(weighted=False, order=3), dict(add_self_loop=False, order=4), dict(add_self_loop=False, order=3, weighted=False),
         dict(normalize_out=True, order=5), dict(normalize_out=True, order=2, add_self_loop=False)]


@pytest.mark.parametrize("kw", MIXED, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_both_regimes_in_one_call(ops, lib, mixed, kw):
    sc, ptr = call_of(mixed)
    kw = dict(kw, eps=1e-3)
    out, mptr, st = markov_twice(ops, sc, ptr, 4097, **kw)
    assert (st["small_tiles"], st["large_tiles"], st["groups"]) == (1 + 2 + 5 + 4, 65, 2)
    assert st["launches"] == (2 + 4) + (1 + kw["order"] + 1 + 4) and st["host_syncs"] == 3
    equals_mirror(lib, out, mptr, mixed, normalize=kw.get("normalize_out", False), **kw)


def test_ids_without_edges_in_both_regimes(ops, lib, bands):
    """(i, i, 0) rows (RLAP_MARKOV_ZERO_ROWS, through the C flags of ops.markov_diffusion's call): with node_ptr, graphs of 3, 130
    and 4,097 ids whose last id has no edges."""
    sizes = [3, 130, 4097]
    node_ptr = np.concatenate([[0], np.cumsum(sizes)])
    eis = [np.asarray(path(2)), np.asarray(path(129)), None]
    b = bands[4097]
    keep = (b[:, 0] < 4096) & (b[:, 1] < 4096)
    eis[2] = b[keep][:, [0, 1]].astype(np.int64).T
    ws = [mm.symmetric_weights(eis[0], 1), mm.symmetric_weights(eis[1], 2), b[keep][:, 2]]
    ei = np.concatenate([e + int(o) for e, o in zip(eis, node_ptr[:-1])], 1)
    t, tw = torch.from_numpy(ei).cuda(), torch.from_numpy(np.concatenate(ws)).cuda()
    for loop in (False, True):
        gi, gw = ops.markov_diffusion(t, tw, int(node_ptr[-1]), node_ptr=node_ptr.tolist(), order=3, eps=1e-3, add_self_loop=loop)
        st = dict(ops.last_stats)
        assert (st["small_tiles"], st["large_tiles"]) == (1 + 3, 65)
        parts = []
        for g in range(3):
            lo = int(node_ptr[g])
            rows = mm.column_layout(eis[g] + lo, ws[g])
            parts.append(np.concatenate([rows, [[node_ptr[g + 1] - 1.0, node_ptr[g + 1] - 1.0, 0.0]]]))
        want, _ = mm.run_call(lib, np.concatenate(parts), np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]), order=3, eps=1e-3,
                              self_loop=loop, zero_ok=True)
        assert torch.equal(gi.cpu(), torch.from_numpy(want[:, :2].astype(np.int64).T.copy()))
        assert same_bits(gw.cpu(), torch.from_numpy(want[:, 2].copy()))
        last = torch.tensor(node_ptr[1:] - 1, device=gi.device)
        assert int(torch.isin(gi[0], last).sum()) == (3 if loop else 0)


# ------------------------------------------------------------------------------------------------ d. groups
def test_groups_by_the_tile_count(ops, lib):
    """65,537 one-tile segments: a group ends at 65,535 tiles, the output offset is carried into the second."""
    S = 65_537
    two = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 2.0]])
    one = torch.from_numpy(two).cuda()
    alone, ap, st1 = markov_twice(ops, one, [0, 2], 2)
    assert ap.tolist() == [0, 4] and (st1["groups"], st1["small_tiles"]) == (1, 1)
    equals_mirror(lib, alone, ap, [two])
    out, mptr, st = markov_twice(ops, one.repeat(S, 1), list(range(0, 2 * S + 1, 2)), 2)
    assert (st["groups"], st["small_tiles"], st["large_tiles"], st["rows_needed"]) == (2, S, 0, 4 * S)
    assert torch.equal(mptr.cpu(), 4 * torch.arange(S + 1))
    assert same_bits(out.reshape(S, 4, 3), alone.unsqueeze(0).expand(S, 4, 3))


# ------------------------------------------------------------------------------------------------ e. the output retry
def test_output_retry(ops, lib, monkeypatch):
    """A star of 2,100 nodes at eps = 1e-6 keeps all 4,410,000 pairs: more than the first capacity, max(16 m + 64, 2^22).  The
    result equals the mirror, and the same call with a first capacity that suffices."""
    n = 2100
    rows = weighted(star(n), 1)
    sc = torch.from_numpy(rows).cuda()
    assert n * n > max(16 * rows.shape[0] + 64, 1 << 22)
    out, mptr = ops.snapshot_markov(sc, [0, sc.shape[0]], n, eps=1e-6)
    st = dict(ops.last_stats)
    assert st["output_retries"] == 1 and st["rows_needed"] == n * n == out.shape[0] and st["first_cap"] == 1 << 22
    equals_mirror(lib, out, mptr, [rows], eps=1e-6)
    monkeypatch.setattr(ops, "PPR_FIRST_CAP_MIN", 1 << 23)
    big, bptr = ops.snapshot_markov(sc, [0, sc.shape[0]], n, eps=1e-6)
    assert ops.last_stats["output_retries"] == 0 and ops.last_stats["first_cap"] == n * n
    assert same_bits(out, big) and torch.equal(mptr, bptr)
    few, _ = ops.snapshot_markov(sc, [0, sc.shape[0]], n, eps=1e-2)
    assert ops.last_stats["output_retries"] == 0 and 0 < few.shape[0] < n * n
