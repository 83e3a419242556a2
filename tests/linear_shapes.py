"""The shapes of the GEMM tests of tests/test_kernels_gpu.py, shared with tests/test_linear_plan_cpu.py, which asks the library
(ops.linear_plan: host-only) which kernel each of them runs.  The kernel named in a comment is what the plan says at default
settings - test_linear_plan_cpu.py holds the whole table and fails when it drifts."""

# test_linear_epilogues: (N, K, O)
EPILOGUE_SHAPES = [
    (300, 512, 512), (1000, 512, 2048), (257, 2048, 512),  # at most one round of 64 x 128 tiles: 8 waves per tile (K split over wave groups)
    (129, 64, 128), (5, 64, 64),  # K = 64 is no whole 128-wide stage: the two-wave 64 x 128 ring kernel
    (70, 20, 64), (50, 11, 7),  # K % 8 != 0: generic (VALU)
    (333, 512, 100), (1030, 64, 100), (1500, 72, 512),  # O % 8 or K % 64 != 0: 128 x 128 register-staged
    (2100, 2048, 512), (1111, 512, 512),  # 64 x 128, 8 waves, ragged last row tile
    (1300, 512, 2048), (4200, 512, 2048), (3000, 192, 3072),  # 192 x 128 ping-pong ring; the last two > 256 tiles: several per workgroup
    (10242, 512, 512),  # 192 x 128 ping-pong ring (216 tiles instead of 164 of 256 rows)
    (10242, 512, 2048), (10242, 192, 2048),  # 160 x 256 big tile, two per CU, + 2 tail rows on the VALU
    (4096, 512, 2048),  # 256 x 128 ping-pong ring: one exact round of 256 tiles
    (5282, 1024, 512),  # narrow 160 x 128 without statistics (33 x 4 tiles, K split over two wave groups) + 2 tail rows
]

# test_linear_concat_and_gather: (N, K1, K2, O); the K-concat call has K = K1 + K2, the gather-add call K = K1
CONCAT_GATHER_SHAPES = [
    (400, 512, 512, 512), (200, 128, 64, 256), (1400, 512, 512, 512), (1200, 128, 64, 256),  # concat: two-wave 64 x 128 ring; gather-add: 8 waves
    (90, 32, 32, 32),  # 128 x 128 register-staged
    (10242, 256, 256, 2048),  # 160 x 256 big tile + 2 tail rows with the K-concat / gather-add epilogue
]

# test_layernorm_folded_into_neighbouring_gemms: row counts of the [N, 2048] -> 512 producer and the [N, 512] -> 2048 consumer.
# 10242: narrow 160 x 128 producer + 2 tail rows without strip sums, 160 x 256 big-tile consumer that recomputes those two rows /
# 640: whole 64-row tiles / 4000: partial last tile, 192 x 128 lock-step consumer / 330: tail of 10 / 5282, 5312 = 320 k + 162 and
# 320 k + 192: <= 32 rows beyond a multiple of 160 but NOT of 320 (the producer used to peel them without strip sums while the consumer
# expected sums; the plain GEMM of the same shape does peel them) / 642, 1469, 2562: small-tile consumers (< 4096 rows)
FOLD_ROWS = [10242, 640, 4000, 330, 5282, 5312, 642, 1469, 2562]
FOLD_D, FOLD_HIDDEN = 512, 2048


def planned_calls():
    """(role, N, K1, K2, O) of every ops.linear / linear_with_row_stats / linear_ln_folded call those three tests make."""
    calls = [("plain", n, k, 0, o) for n, k, o in EPILOGUE_SHAPES]
    for n, k1, k2, o in CONCAT_GATHER_SHAPES:
        calls += [("plain", n, k1, k2, o), ("plain", n, k1, 0, o)]
    for n in FOLD_ROWS:
        calls += [("stats_producer", n, FOLD_HIDDEN, 0, FOLD_D), ("plain", n, FOLD_HIDDEN, 0, FOLD_D), ("fold_consumer", n, FOLD_D, 0, FOLD_HIDDEN)]
    return calls
