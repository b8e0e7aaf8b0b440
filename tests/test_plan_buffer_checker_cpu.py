"""The checker of tests/test_gpu_plan_buffer.py without a GPU: check_buffer runs against a stand-in for `ops` whose plans are
assembled on the host -- the lists by tests/csrc/plan_mirror.cc (the layout rules of rlap_plan.h), the coefficients by the torch
formulation of tests/test_gpu_propagate.py in the entry order ops.snapshot_gcn_norm documents -- and laid out by plan_layout.  A
clean plan passes every check; a plan with a zero word set, or with a directory whose chunk numbers are one too high, is refused
with a message that names the part.  So the device test's checker is known to work, and to notice, before it meets a device."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import plan_buffer
import test_gpu_plan_buffer as device_test
from test_gpu_plan import HAND, star
from test_gpu_propagate import flags_of, segments, torch_segment
from test_plan_cpu import libs  # noqa: F401  (a fixture)

C = 256


class HostOps:
    """ops.snapshot_plan / snapshot_gcn_norm / debug_set_poison as far as check_buffer uses them."""

    def __init__(self, lib, defect=None):
        self.lib, self.defect, self.poison = lib, defect, 0

    def debug_set_poison(self, byte):
        self.poison = byte

    def snapshot_gcn_norm(self, sc, ptr, n, node_ptr=None, dtype=torch.float64, **kw):
        srcs, dsts, vals, e = [], [], [], [0]
        for s, l, lo, hi, r0, r1 in segments(ptr, n, node_ptr):
            a, b, v = torch_segment(sc[r0:r1], lo, hi, **flags_of(kw))
            srcs.append(a)
            dsts.append(b)
            vals.append(v)
            e.append(e[-1] + a.numel())
        return torch.stack([torch.cat(srcs), torch.cat(dsts)]), torch.cat(vals), torch.tensor(e)

    def snapshot_plan(self, sc, ptr, n, node_ptr=None, directions="both", **kw):
        lib = self.lib
        rows = np.ascontiguousarray(sc.double().numpy())
        p = np.array(torch.as_tensor(ptr).tolist(), dtype=np.int64)
        m, S = rows.shape[0], len(p) - 1
        G = len(node_ptr) - 1 if node_ptr is not None else 1
        slots = (S // G) * n
        loops = kw.get("add_self_loops", True)
        val = self.snapshot_gcn_norm(sc, ptr, n, node_ptr=node_ptr, **kw)[1].numpy()
        row_at, loop_at, _ = plan_buffer.entry_numbers(rows, p.tolist(), n, G, node_ptr, loops)
        c = np.where(row_at >= 0, val[np.maximum(row_at, 0)], 0.0) if m else np.zeros(0)
        want = {"forward": directions in ("both", "forward"), "transposed": directions in ("both", "transposed")}
        L = np.zeros(8, dtype=np.int64)
        lib.plan_layout(m, slots, int(loops), int(want["forward"]), int(want["transposed"]), L.ctypes.data)
        L = dict(zip(("loop", "off_forward", "off_transposed", "dir_forward", "dir_transposed", "rec_forward", "rec_transposed", "bytes"), L.tolist()))
        buf = np.full(L["bytes"], self.poison & 0xFF, dtype=np.uint8)           # what the build does not write keeps the poison

        def put(offset, array):
            b = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
            buf[offset:offset + b.size] = b

        flags = (plan_buffer.GCN_SELF_LOOPS if loops else 0) | (4 if kw.get("normalize", True) else 0)
        desc = SimpleNamespace(m=m, segments=S, graphs=G, num_nodes=n, loop_offset=L["loop"], magic=0x504C414E)
        if loops:
            put(L["loop"], val[loop_at])
        info = {"entries": 0, "loops_removed": int((row_at < 0).sum())}
        used, cap = 256, lib.plan_dir_cap(m)
        for t, (name, bit) in enumerate(plan_buffer.DIRECTIONS):
            for part in ("off_", "dir_", "rec_"):
                setattr(desc, part + name, L[part + name])
            if not want[name]:
                setattr(desc, "entries_" + name, -1)
                setattr(desc, "chunks_" + name, -1)
                info["chunked_lists_" + name] = -1
                continue
            flags |= bit
            off = np.zeros(slots + 1, dtype=np.int64)
            rec_c, rec_id = np.zeros(max(m, 1)), np.zeros(max(m, 1), dtype=np.int32)
            dslot, dk = np.zeros(max(cap, 1), dtype=np.int64), np.zeros(max(cap, 1), dtype=np.int64)
            chunks = ctypes.c_int64(0)
            ent = lib.plan_build(m, rows.ctypes.data, S, p.ctypes.data, G, n, c.ctypes.data, int(loops), t, off.ctypes.data, rec_c.ctypes.data,
                                 rec_id.ctypes.data, dslot.ctypes.data, dk.ctypes.data, ctypes.byref(chunks))
            assert ent >= 0
            put(L["off_" + name], off)
            ref = np.zeros(chunks.value, dtype=plan_buffer.CHUNKREF)
            ref["slot"], ref["k"] = dslot[:chunks.value], dk[:chunks.value]
            if self.defect == "directory":
                ref["k"] += 1
            put(L["dir_" + name], ref)
            rec = np.zeros(ent, dtype=plan_buffer.RECORD)
            rec["c"], rec["id"] = rec_c[:ent], rec_id[:ent]
            if self.defect == "zero":
                rec["zero"] = 1
            put(L["rec_" + name], rec)
            setattr(desc, "entries_" + name, ent)
            setattr(desc, "chunks_" + name, chunks.value)
            info["chunked_lists_" + name] = len(set(dslot[:chunks.value].tolist()))
            info["entries"] = ent + (slots if loops else 0)
            used = max(used, L["rec_" + name] + 16 * ent, L["dir_" + name] + 16 * cap)
        used = (used + 255) // 256 * 256
        desc.flags, desc.plan_bytes = flags, used
        return SimpleNamespace(buffer=torch.from_numpy(buf[:used].copy()), desc=desc, info=info, nbytes=used, entries=info["entries"],
                               layers=S // G, num_nodes=n)


def run_inputs(ops):
    rows = torch.tensor(HAND, dtype=torch.float64)
    two = torch.cat([rows, rows])
    leaves = 2 * C + 40
    a = star(leaves, 4, loops=[(3, 2.5), (C, 0.75), (C + 20, 1.25)])
    stars = torch.from_numpy(np.concatenate([a, star(leaves, 5)]))
    for w in (False, True):
        device_test.check_buffer(ops, C, two, [0, 8, 16], 7, "hand-built twice", weighted=w)
        device_test.check_buffer(ops, C, two, [0, 0, 8, 8, 16, 16], 7, "hand-built with empty segments", weighted=w, fill_value=2.0)
        device_test.check_buffer(ops, C, two, [0, 8, 16], 7, "hand-built, loops kept", weighted=w, add_self_loops=False)
        device_test.check_buffer(ops, C, two, [0, 8, 16], 7, "hand-built, weights as they are", weighted=w, normalize=False)
        for directions in ("both", "forward", "transposed"):
            device_test.check_buffer(ops, C, stars, [0, len(a), len(a) + 2 * leaves], leaves + 3, "stars with loop rows", directions=directions, weighted=w)
    device_test.check_buffer(ops, C, torch.zeros((0, 3), dtype=torch.float64), [0, 0, 0], 5, "m = 0")
    g0, g1 = [[1, 0, 1.0], [0, 1, 1.5], [2, 1, 0.5], [1, 2, 0.5]], [[4, 3, 2.0], [3, 4, 2.0]]    # two graphs a layer, two layers
    batch = torch.tensor(g0 + g1 + g0 + g1, dtype=torch.float64)
    device_test.check_buffer(ops, C, batch, [0, 4, 6, 10, 12], 5, "node_ptr batch", node_ptr=[0, 3, 5], weighted=True)


def test_checker_accepts_a_plan_assembled_on_the_host(libs):
    assert libs[1].spmm_chunk() == C
    run_inputs(HostOps(libs[0]))


@pytest.mark.parametrize("defect, part", [("zero", "zero words"), ("directory", "the directory")])
def test_checker_names_a_seeded_defect(libs, defect, part):
    with pytest.raises(AssertionError, match=part):
        run_inputs(HostOps(libs[0], defect))
