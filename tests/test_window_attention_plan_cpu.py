"""CPU checks of the window attention's band arithmetic (csrc/window_attention_core.h) through its host-only query,
ops.window_attention_plan -> anemoi_window_attention_plan: which tiles a wave of the forward, the backward's query pass and its key pass
visits, skips and runs without masks.  Brute force against the definition of the band, for every block, wave and tile.  No GPU: the query
launches nothing."""
import pytest
import torch

from anemoi_core_amd import _lib, ops

SEQ_LENS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)
WAVES, STRIP, OWN = 4, 16, 64


def windows(N):
    return (0, 1, 7, 31, 32, 33, 63, 64, 65, -1, N - 2, N - 1, N)


def in_band(i, j, N, w):
    """The definition: both rows exist and are within w of each other (w < 0: unbounded)."""
    return i < N and j < N and (w < 0 or abs(i - j) <= w)


# (pass, d) -> tile rows: both tile sizes of the family (the key pass halves its tile at d = 128)
TILINGS = (("forward", 64, 64), ("backward_query", 64, 64), ("backward_key", 64, 64), ("backward_key", 128, 32))


@pytest.mark.parametrize("op,d,tile_rows", TILINGS, ids=[f"{op}-d{d}" for op, d, _ in TILINGS])
def test_every_tile_class_agrees_with_the_band_by_brute_force(op, d, tile_rows):
    combos = 0
    for N in SEQ_LENS:
        for window in windows(N):
            w = -1 if window < 0 or window >= N - 1 else window  # the normalisation, from its definition
            blocks = -(-N // OWN)
            covered = set()
            for block in range(blocks):
                for wave in range(WAVES):
                    p = ops.window_attention_plan(op, N, d, window, block=block, wave=wave)
                    assert (p.window, p.rows_per_block, p.grid_x, p.tile_rows) == (w, OWN, blocks, tile_rows), (N, window, block, wave)
                    assert 0 <= p.lo <= p.hi <= N and p.ntiles == -(-(p.hi - p.lo) // tile_rows) == len(p.tiles)
                    strip = range(block * OWN + wave * STRIP, block * OWN + (wave + 1) * STRIP)
                    for t, cls in enumerate(p.tiles):
                        combos += 1
                        tile = range(p.lo + t * tile_rows, p.lo + (t + 1) * tile_rows)
                        pairs = [in_band(i, j, N, w) for i in strip for j in tile]
                        if cls == "skipped":
                            assert not any(pairs), (N, window, block, wave, t)
                        elif cls == "full":
                            assert all(pairs), (N, window, block, wave, t)
                        else:
                            assert cls == "masked"
                            # a visited tile's rows from `hi` on are read as zeros: no in-band pair may lie there
                            assert not any(in_band(i, j, N, w) for i in strip for j in tile if j >= p.hi), (N, window, block, wave, t)
                        if cls != "skipped":
                            covered.update((i, j) for i in strip for j in tile if j < p.hi)
            # every pair of the band with an existing owned row lies in a visited tile, below hi
            want = {(i, j) for i in range(N) for j in range(N) if in_band(i, j, N, w)}
            assert want <= covered, (N, window, sorted(want - covered)[:4])
    assert combos > 1000


def test_the_lists_hold_4660_block_wave_tile_combinations_over_both_tile_sizes():
    def count(op, d):
        return sum(len(ops.window_attention_plan(op, N, d, window, block=b, wave=wv).tiles)
                   for N in SEQ_LENS for window in windows(N) for b in range(-(-N // OWN)) for wv in range(WAVES))

    assert (count("forward", 64), count("backward_key", 128)) == (1756, 2904)  # 64-row and 32-row tiles: 4660 together


def test_fp32_rows_own_their_band_alone():
    """The plain kernels: one row per workgroup, every 64-lane tile of [lo, hi) visited, the last one partial unless it ends on hi."""
    for N, window in ((1, 0), (65, 7), (200, 64), (200, -1), (129, 200)):
        w = -1 if window < 0 or window >= N - 1 else window
        for op in ops.WINDOW_PASSES:
            for i in (0, N // 2, N - 1):
                p = ops.window_attention_plan(op, N, 32, window, dtype=torch.float32, block=i)
                band = [j for j in range(N) if in_band(i, j, N, w)]
                assert (p.rows_per_block, p.grid_x, p.tile_rows, p.lo, p.hi) == (1, N, 64, band[0], band[-1] + 1)
                assert p.tiles == ("full",) * ((p.hi - p.lo) // 64) + ("masked",) * ((p.hi - p.lo) % 64 != 0)


def test_refusals():
    with pytest.raises(NotImplementedError, match="head dimension 48 not supported; supported: 32, 64, 128"):
        ops.window_attention_plan("forward", 100, 48, 4)
    with pytest.raises(ValueError, match="no block 2, wave 0"):
        ops.window_attention_plan("forward", 100, 64, 4, block=2)
    with pytest.raises(ValueError, match="no block 0, wave 4"):
        ops.window_attention_plan("backward_key", 100, 64, 4, wave=4)
    with pytest.raises(ValueError, match="no block 0, wave 1"):
        ops.window_attention_plan("forward", 100, 64, 4, dtype=torch.float32, wave=1)
    with pytest.raises(ValueError, match="bad sizes"):
        ops.window_attention_plan("forward", -1, 64, 4)
    lib = _lib.load()
    assert lib.anemoi_window_attention_plan(3, 100, 64, 4, _lib.BF16, 0, 0, _lib.WindowAttentionPlan(), None, 0) == _lib.E_INVALID
    assert b"unknown pass 3" in lib.anemoi_hip_last_error()
    sizes = _lib.WindowAttentionPlan()  # the sizes alone, without a class buffer
    assert lib.anemoi_window_attention_plan(0, 200, 64, 7, _lib.BF16, 1, 2, sizes, None, 0) == 0
    assert (sizes.lo, sizes.hi, sizes.ntiles) == (57, 135, 2)
    assert ops.window_attention_plan("forward", 0, 64, 4).tiles == ()
