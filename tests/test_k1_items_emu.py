"""CPU check of the tiled cutter's bounded item list (K1, csrc/skm_tile.hpp: tile_put_items, tile_item_run,
tile_item_cap, tile_list_items, tile_plan) through the serial harness tests/emu_k1_items.cpp: phase B with immediate items, the barrier,
phase E from the item, the overflow flag and the slow turns -- the records of every tile against skm_split_read +
skm_make_record as a multiset.  The harness is a stand-alone program built with the address and undefined-behaviour
sanitizers; its list rows have exactly the kernel's sizes, so a store past the list aborts it."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu_k1_items") / "emu_k1_items")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "emu_k1_items.cpp"), "-o", exe])
    return exe


def run(prog, K, length, n_reads, R, forced, ragged=0, dense=0, mer127=0):
    p = subprocess.run([prog] + [str(x) for x in (K, length, n_reads, R, forced, ragged, dense, mer127)], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    return p.stdout


# forced: 0 = the list as launch_tiled sizes it, 1 = PG_K1_ITEM_CAP=1, -1 = exactly each tile's items (fits), -2 = one fewer (overflows)
@pytest.mark.parametrize("forced", [0, 1, -1, -2])
@pytest.mark.parametrize("K,length,R,mer127", [(21, 150, 16, 0), (63, 150, 32, 0), (127, 150, 32, 1), (31, 100, 28, 0)])
def test_items_match_serial_walk(prog, K, length, R, mer127, forced):
    """Tiles of 1, R - 1 and R reads (n_reads = 1, R - 1, R, and 2 R + 1: a full tile, then a short one)."""
    for n_reads in (1, R - 1, R, 2 * R + 1):
        out = run(prog, K, length, n_reads, R, forced, mer127=mer127)
        if forced in (1, -2) and n_reads >= R - 1 and K != 127:
            assert " 0 of " not in out                        # the slow path was taken
        if forced in (0, -1):
            assert " 0 of " in out                            # ... and was not


@pytest.mark.parametrize("forced", [0, 1, -1, -2])
@pytest.mark.parametrize("K,length,R,mer127", [(21, 150, 16, 0), (63, 150, 24, 0), (127, 150, 32, 1)])
def test_items_ragged_lengths(prog, K, length, R, mer127, forced):
    """Lengths from K + 1 (the first read) up to the bound (the second), the rest in between."""
    run(prog, K, length, 3 * R + 5, R, forced, ragged=1, mer127=mer127)


@pytest.mark.parametrize("forced", [0, 1, -1, -2])
def test_items_dense_starts(prog, forced):
    """No read makes EVERY k-mer start a run (the minimizer would have to move at every step: m-mer values rising or falling
    strictly all along the read, and a greedy choice of bases runs out of room in 32 bits within some twenty steps).  The
    generator takes the base that starts a run wherever one of the four does: at K = 21 (w = 7) that reaches about 0.34 starts
    a k-mer against 0.26 of random reads -- 39 records a read -- which the harness prints."""
    out = run(prog, 21, 150, 40, 16, forced, dense=1)
    assert float(out.split("densest read ")[1].split()[0]) > 0.3


@pytest.mark.parametrize("forced", [0, 1, -1, -2])
@pytest.mark.parametrize("K,length,n_reads,mer127", [(31, 100, 70, 0), (63, 150, 70, 0), (127, 150, 70, 1), (63, 4000, 3, 0)])
def test_items_on_the_products_tiles(prog, K, length, n_reads, mer127, forced):
    """R = 0: the segment length and the reads a tile that tile_plan gives launch_tiled for the geometry (100 bp, K = 31: S = 9, not
    tile_pick_segment's 7).  4000 bases at K = 63: one read a tile, more segments than a workgroup has threads -- the kernel's phase B
    takes two rounds there, which in this serial harness is one loop; the GPU test of that length runs the rounds."""
    out = run(prog, K, length, n_reads, 0, forced, mer127=mer127)
    if (K, length) == (31, 100):
        assert " S 9 " in out and " R 32 " in out
    if length == 4000:
        assert " R 1 " in out
