"""The tile and group table of the PPR diffusion (rlap_amd/csrc/rlap_ppr_tiles.h, step 4 of snapshot_ppr_run) without a
GPU: tests/csrc/ppr_tiles_main.cc, a stand-alone program under -fsanitize=address,undefined, checks for every list of segment sizes
below -- with bcap equal to the sum of the sizes and larger -- that both copies of every tile lie inside the tile area, that tiles of
a group do not overlap, that ROFF ascends from 0 in steps of n_s, that a group's rows are the sum of its tiles' and fit the per-row
counters, that the tiles fit the table, that no group holds more than 65,535 tiles or (with more than one tile) exceeds the budget,
that the small regime's tiles come first, that every (segment, c0) occurs exactly once and that the tile counts match a recount.
The counts the program prints are compared with a recount in Python."""
import itertools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, SMALL_MAX, BUDGET, GROUP_TILES = 64, 4096, 1 << 30, 65535
EDGE_SIZES = [0, 1, 63, 64, 65, 4095, 4096, 4097]


def lists():
    out = [list(c) for k in range(4) for c in itertools.product(EDGE_SIZES, repeat=k)]
    out += [[2] * 70_000, [4096] * 5, [4100] * 4, [1_100_000], [1_100_000] + [100] * 10, [100] * 10 + [1_100_000]]
    rng = np.random.RandomState(20)
    for _ in range(300):                                 # the three scales mixed: a few nodes, around the regime edge, near the budget
        k = rng.randint(1, 40)
        scale = rng.choice(3, size=k, p=[0.6, 0.3, 0.1])
        small = rng.randint(0, 200, size=k)
        edge = rng.randint(3900, 4300, size=k)
        big = rng.randint(20_000, 300_000, size=k)
        out.append(np.where(scale == 0, small, np.where(scale == 1, edge, big)).tolist())
    return out


def recount(sizes):
    """(tiles, groups, small tiles, large tiles, largest group's rows) by the rules of DESIGN 4.8, written out again."""
    tiles = groups = small = large = max_rows = 0
    for regime in (True, False):
        live = count = rows = 0
        opened = False
        for n in sizes:
            if n == 0 or (n <= SMALL_MAX) != regime:
                continue
            for _ in range(-(-n // TILE)):
                if not opened or live + 1024 * n > BUDGET or count == GROUP_TILES:
                    groups += 1
                    live = count = rows = 0
                    opened = True
                live += 1024 * n
                count += 1
                rows += n
                max_rows = max(max_rows, rows)
                tiles += 1
                small += regime
                large += not regime
    return tiles, groups, small, large, max_rows


def test_the_tile_table_under_asan_ubsan(tmp_path):
    exe = tmp_path / "ppr_tiles"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "ppr_tiles_main.cc")])
    ls = lists()
    assert len(ls) == 585 + 6 + 300
    text = "".join(" ".join(map(str, [len(l)] + l)) + "\n" for l in ls)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"{len(ls)} lists, 0 failures" in r.stdout
    got = [tuple(map(int, ln.split()[1:])) for ln in r.stdout.splitlines() if ln.startswith("list ")]
    assert len(got) == len(ls)
    for l, g in zip(ls, got):
        assert g == recount(l), l[:10]
    by = {tuple(l): g for l, g in zip(ls, got) if len(l) < 20 or len(set(l)) == 1}
    # the shapes tests/test_gpu_ppr_regimes.py runs on the device, and a single tile larger than the budget
    assert by[(4096,) * 5][:4] == (320, 2, 320, 0)
    assert by[(4100,) * 4][:4] == (260, 2, 0, 260)
    assert by[(2,) * 70_000][:4] == (70_000, 2, 70_000, 0)
    assert by[(1_100_000,)][:4] == (17_188, 17_188, 0, 17_188)
    assert by[(1_100_000,) + (100,) * 10][:4] == (17_188 + 20, 17_188 + 1, 20, 17_188)
    assert by[(4096, 4097)][:4] == (64 + 65, 2, 64, 65)
