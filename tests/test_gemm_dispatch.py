"""The GEMM tile rule lives in ONE place, the library's resolver (mh_gemm_bf16_resolve_tile, csrc/gemm.hip): what it answers for
MH_TILE_AUTO, for explicit tiles and through the host-side A/B switches of maestro_amd/hip.py.  No GPU needed: nothing is launched.

The expected tiles are RECORDED, not computed: they were produced at the commit before the resolver existed by running its
Python copy of the rule (``hip._auto_tile_name`` / ``hip._pick_tile``) on these rows.  Where that copy disagreed with the C
dispatch it mirrored, the row is marked "C:" and its value was worked out by hand from the C code of that commit (the kernel that
was launched, which is what the resolver must name)."""

import pytest

from maestro_amd import hip

NT, NN, TN = hip.GEMM_NT, hip.GEMM_NN, hip.GEMM_TN
PLAIN = 0
FC1 = hip.BIAS | hip.GELU | hip.AUX_DGELU | hip.AUX_U8      # fc1 forward: bias, GELU, byte-coded GELU' saved
F32RES = hip.OUT_F32 | hip.BIAS | hip.RESIDUAL              # out-proj / fc2 forward: fp32 residual stream
DFC2 = hip.MULAUX | hip.AUX_U8 | hip.COLSUM                 # fc2 dgrad: times GELU', column sums for the fc1 bias gradient
WGRAD = hip.ATOMIC | hip.OUT_F32                            # weight gradients: split-K, fp32 atomics
R, D, P, W, L, AUTO = hip.TILE_REG_128, hip.TILE_DMA_256, hip.TILE_PP_128, hip.TILE_REG_192, hip.TILE_DMA_256_LOCKSTEP, hip.TILE_AUTO
CODE = {"R": R, "D": D, "P": P, "W": W, "L": L, "A": AUTO}


def packed(layout, M, N, K, flags):  # noqa: N803
    """Leading dimensions of packed operands: lda, ldb, ldc, ldr, ldaux."""
    return (M if layout == TN else K, K if layout == NT else N, N, N if flags & hip.RESIDUAL else 0,
            N if flags & (hip.GELU | hip.MULAUX) else 0)


def resolve(layout, M, N, K, flags, tile=AUTO, families=hip.FAMILY_ALL):  # noqa: N803
    return hip.resolve_tile(tile, layout, M, N, K, *packed(layout, M, N, K, flags), flags, families)


# ---- MH_TILE_AUTO on the training step's signatures: one letter per (N, K), N-major, for every M
STEP_M = (3200, 8192, 11392, 12800, 32768, 557056)
STEP_N = (512, 768, 1536, 2304, 3072)
STEP_K = (512, 768, 1536, 3072)
# C: M = 557056 with K = 3072 -- the A operand spans 557056 x 3072 x 2 B = 3.4 GB, beyond the 2 GiB a buffer descriptor addresses: the
# ping-pong and LDS-DMA launches both declined and the register tile ran.  The Python copy knew no reach test and said DMA_256.
SEG = "DDDRDDDRDDDRDDDRDDDR"
STEP_AUTO = {
    (NT, PLAIN): ("RRRRRRRRPPPPPPPPPPPP", "PPPPPPPPPPPPPPPPPPPP", "PPPPPPWWPPPPPPPPPPPP", "PPPPPPPPPPPPPPPPPPPP", "PPDDPPPPPPDDPPDDPPDD", SEG),
    (NT, FC1): ("RRRRRRRRPPPPPPPPPPPP", "PPPPPPPPPPPPPPPPPPPP", "PPPPPPWWPPPPPPPPPPPP", "PPPPPPPPPPPPPPPPRRRR", "PPPPPPPPDDDDDDDDDDDD", SEG),
    (NT, F32RES): ("RRRRRRRRPPPPPPPPPPPP", "PPPPPPPPPPPPPPPPPPPP", "PPPPPPWWPPPPPPPPPPPP", "PPPPPPPPPPPPPPPPPPPP", "PPDDPPPPPPDDPPDDPPDD", SEG),
    (NN, PLAIN): ("RRRRRRRRRRRRRRRRRRRR", "RRRRRRRRRRRRRRRRRRRR", "RRRRRRWWRRRRRRRRRRRR", "RRRRRRRRRRRRRRRRRRRR", "DDDDRRRRDDDDDDDDDDDD", SEG),
    (NN, DFC2): ("RRRRRRRRRRRRRRRRRRRR", "RRRRRRRRRRRRRRRRRRRR", "RRRRRRRRRRRRRRRRRRRR", "RRRRRRRRRRRRRRRRRRRR", "DDDDRRRRDDDDDDDDDDDD", SEG),
    (TN, WGRAD): ("RRRRRRRRRRRRRRRRRRRR",) * 6,
}
STEP_ROWS = [(layout, M, N, K, flags, CODE[row[i]]) for (layout, flags), rows in STEP_AUTO.items() for M, row in zip(STEP_M, rows)
             for i, (N, K) in enumerate((N, K) for N in STEP_N for K in STEP_K)]

# ---- MH_TILE_AUTO on both sides of every constant of the rule.  t128 / t192 / t256 = tiles of 128 x 128 / 192 x 128 / 256 x 256
EDGE_ROWS = [
    (NT, 200, 72, 104, PLAIN, R),              # tiny, K tail
    (NT, 2048, 2048, 512, PLAIN, P), (NT, 2048, 2048, 512, FC1, P), (NT, 2048, 2048, 512, F32RES, P),
    (NN, 2048, 2048, 512, PLAIN, R),           # the ping-pong tile is picked for NT only
    (NT, 4096, 4096, 256, PLAIN, D), (NN, 4096, 4096, 256, PLAIN, D),          # t256 = 256, K < 512: no ping-pong
    (NT, 11392, 768, 1536, PLAIN, W), (NN, 11392, 768, 1536, PLAIN, W),        # t128 = 534, t192 = 360
    (NT, 2048, 1920, 512, PLAIN, R),           # t128 = 240
    (NT, 2048, 1984, 512, PLAIN, R),           # t128 = 256 but N % 128 != 0: no ping-pong
    (NT, 2048, 2048, 448, PLAIN, R), (NT, 2048, 2048, 512, PLAIN, P),          # ping-pong K >= 512
    (NT, 32640, 128, 512, PLAIN, R), (NT, 32768, 128, 512, PLAIN, P),          # t128 = 255 / 256
    (NN, 32768, 256, 1536, PLAIN, R), (NN, 21888, 384, 1536, PLAIN, W),        # t128 = 512 / 513
    (NN, 65664, 128, 1536, PLAIN, W),                                           # t128 = 513 with t256 = 257 (two waves at 50 %: no DMA)
    (NN, 24576, 384, 1536, PLAIN, W), (NN, 73728, 128, 1536, PLAIN, W), (NN, 73856, 128, 1536, PLAIN, R),   # t128 = 576 / 576 / 577
    (NN, 384, 24320, 1536, PLAIN, W), (NN, 256, 35840, 1536, PLAIN, R),        # t128 = 570 / 560 with t192 = 380 / 560 (> 512)
    (NT, 11392, 768, 1472, PLAIN, P), (NN, 11392, 768, 1472, PLAIN, R),        # 192-row K >= 1536 (against the 1536 rows above)
    (NT, 294912, 128, 512, FC1, P), (NT, 295040, 128, 512, FC1, D),            # GELU: t128 = 2304 / 2305
    (NT, 1048576, 128, 512, PLAIN, P), (NT, 1048704, 128, 512, PLAIN, D),      # DMA-sized, short K: t128 = 8192 / 8193
    (NT, 32768, 2048, 960, PLAIN, P), (NT, 32768, 2048, 1024, PLAIN, D),       # DMA-sized: ping-pong keeps K < 1024
    (NT, 65280, 256, 2048, PLAIN, P), (NT, 65536, 256, 2048, PLAIN, D),        # t256 = 255 / 256
    (NN, 65280, 256, 2048, PLAIN, R), (NN, 65536, 256, 2048, PLAIN, D),
    (NN, 117760, 256, 2048, PLAIN, R), (NN, 118016, 256, 2048, PLAIN, D),      # t256 = 460 / 461 of 512 slots: 89.8 % / 90.04 %
    (TN, 2048, 2048, 512, PLAIN, R), (TN, 2048, 2048, 512, WGRAD, R), (TN, 4096, 4096, 32768, WGRAD, R),   # TN: the register tile
    # K % 64 == 32 with a K-minor operand.  C: the ping-pong tile (K steps of 64) declines; the LDS-DMA ring steps K by 32
    # (csrc/gemm_ring.hpp BK = 32, "K % 32 != 0 with a K-minor operand" in the header), so K = 288 qualifies and the 256 x 256
    # tile runs where prefer_dma holds.  The Python copy agreed on these rows.
    (NT, 4096, 4096, 288, PLAIN, D), (NN, 4096, 4096, 288, PLAIN, D),
    (NT, 2048, 2048, 288, PLAIN, R),           # too few tiles for the DMA tile, K tail for the ping-pong tile: general path
    (NT, 4096, 4096, 264, PLAIN, R),           # K % 32 != 0: no DMA
]


@pytest.mark.parametrize("rows", [STEP_ROWS, EDGE_ROWS], ids=["step_signatures", "rule_constants"])
def test_auto_rule(rows):
    assert len(STEP_ROWS) == 6 * 6 * 5 * 4
    wrong = [(row, got) for row in rows if (got := resolve(*row[:5])) != row[5]]
    assert not wrong, f"(layout, M, N, K, flags, expected), resolved: {wrong[:8]} ({len(wrong)} rows)"


def test_explicit_tiles():
    for tile in (hip.TILE_REG_64, hip.TILE_REG_192):
        assert resolve(NT, 8192, 768, 768, PLAIN, tile) == tile
        assert resolve(NN, 8192, 768, 768, PLAIN, tile) == tile
        assert resolve(TN, 768, 768, 8192, WGRAD, tile) == R           # K-major A: the 128-row tile runs
        assert resolve(NN, 8192, 768, 3072, DFC2, tile) == R           # column sums: the 128-row tile runs
    assert resolve(NT, 200, 72, 104, PLAIN, R) == R
    assert resolve(NT, 2048, 2048, 512, PLAIN, P) == P and resolve(NN, 2048, 2048, 512, DFC2, P) == P
    assert resolve(NT, 2048, 2048, 448, PLAIN, P) == -2                # K < 512
    assert resolve(NT, 2048, 1984, 512, PLAIN, P) == -2                # N % 128 != 0
    assert resolve(NT, 2048, 1920, 512, PLAIN, P) == P                 # (1920 = 15 x 128: served, as the launch always did)
    assert resolve(NT, 2048, 2048, 512, hip.BIAS, P) == -2             # a flag set the ping-pong tile does not serve
    assert resolve(TN, 2048, 2048, 512, PLAIN, P) == -2
    assert resolve(NT, 557056, 512, 3072, PLAIN, P) == -2 and resolve(NT, 557056, 512, 3072, PLAIN, D) == -2   # beyond 2 GiB
    for tile in (D, hip.TILE_DMA_256x128, hip.TILE_DMA_128x256, hip.TILE_DMA_128, hip.TILE_DMA_128x4, L):
        assert resolve(NT, 200, 128, 128, PLAIN, tile) == tile         # DMA tiles take any size with whole K steps of 32
        assert resolve(NT, 4096, 4096, 288, PLAIN, tile) == tile       # ... K = 288 included (C: BK = 32 in csrc/gemm_ring.hpp)
        assert resolve(NT, 4096, 4096, 264, PLAIN, tile) == -2         # K tail inside a K-minor operand
        assert resolve(NN, 4096, 4096, 264, PLAIN, tile) == -2
        assert resolve(TN, 4096, 4096, 264, WGRAD, tile) == tile       # both operands K-major: zero-filled beyond K
    for diag in range(1, 6):                                           # ablation builds are not in the shipped library
        assert resolve(NT, 2048, 2048, 512, FC1, hip.TILE_PP_128 + diag) == -2


def test_invalid_arguments_are_errors_of_the_gemm_checks():
    with pytest.raises(hip.HipExtensionError, match="mh_gemm_bf16: layout 3"):
        resolve(3, 2048, 2048, 512, PLAIN)
    with pytest.raises(hip.HipExtensionError, match="lda/ldb must be multiples of 8"):
        hip.resolve_tile(AUTO, NT, 2048, 2048, 512, 516, 512, 2048, 0, 0, PLAIN)
    with pytest.raises(hip.HipExtensionError, match="residual epilogue needs f32 output"):
        resolve(NT, 2048, 2048, 512, hip.RESIDUAL)
    for sk in hip.SK_TILES:                                            # stream-K ids belong to mh_gemm_bf16_sk
        with pytest.raises(hip.HipExtensionError, match=f"mh_gemm_bf16: tile {sk}"):
            resolve(NT, 8192, 768, 3072, PLAIN, sk)
    with pytest.raises(hip.HipExtensionError, match="family"):
        resolve(NT, 2048, 2048, 512, PLAIN, AUTO, 8)


# ---- the host-side switches: hip._pick_tile on the step's signatures.  The DMA-only rule (MH_GEMM_PP=0; MH_DMA_STAGGER=0 asks where it
# says DMA_256) gave the same row for every flag set of a layout.  C: K = 3072 at M = 557056 as above -- the Python copy returned
# DMA_256 / its lockstep form there and the launch fell back to the register tile after the library's -2.
DMA_ONLY = {NT: ("R" * 20,) * 4 + ("DDDDRRRRDDDDDDDDDDDD", SEG), NN: ("R" * 20,) * 4 + ("DDDDRRRRDDDDDDDDDDDD", SEG), TN: ("R" * 20,) * 6}


def pick(layout, M, N, K, flags):  # noqa: N803
    lda, ldb, ldc, ldr, ldaux = packed(layout, M, N, K, flags)
    return hip._pick_tile(layout, M, N, K, flags, (layout, M, N, K, None, lda, None, ldb, None, ldc, flags, None, None, ldr, None, None,
                                                   ldaux, None))


@pytest.mark.parametrize("switch", ["MH_GEMM_PP=0", "MH_GEMM_DMA=0", "MH_GEMM_DMA=1", "MH_DMA_STAGGER=0", "MH_GEMM_TILE=3"])
def test_switches_pick_what_they_picked(monkeypatch, switch):
    for name in ("MH_GEMM_PP", "MH_GEMM_DMA", "MH_DMA_STAGGER", "MH_GEMM_TILE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(hip, "_tile_choice", {})
    monkeypatch.setenv(*switch.split("="))
    wrong = []
    for (layout, flags) in STEP_AUTO:
        for M, row in zip(STEP_M, DMA_ONLY[layout]):
            for i, (N, K) in enumerate((N, K) for N in STEP_N for K in STEP_K):
                dma_rule = CODE[row[i]]
                want = {"MH_GEMM_PP=0": dma_rule, "MH_GEMM_DMA=0": R, "MH_GEMM_DMA=1": AUTO if layout == TN else D,
                        "MH_DMA_STAGGER=0": L if dma_rule == D else AUTO, "MH_GEMM_TILE=3": hip.TILE_DMA_128x256}[switch]
                if (got := pick(layout, M, N, K, flags)) != want:
                    wrong.append(((layout, M, N, K, flags), want, got))
    assert not wrong, f"{wrong[:8]} ({len(wrong)} signatures)"
