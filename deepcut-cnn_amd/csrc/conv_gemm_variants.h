// conv_gemm_variants.h — the tile rows of the gather-GEMM, once: first the float32 / float16 table (kVariants of conv_gemm.cpp, row i is
// variant i), then the bfloat16 one (kVariantsBf16, row i is variant kBf16Variant0 + i).  Every row names its element type through one
// of DC_ROW_F32, DC_ROW_F16, DC_ROW_BF16 (NAME, BM, BN, BK, WR, WC, WK, PF, DMA, SWP, WITH_MC), which the including file defines and
// this file undefines at its end: conv_gemm.cpp makes table entries of them (one table per inclusion, the other table's types defined
// empty), conv_gemm_{f32,f16,bf16}.hip the kernel instantiations of their type.  No include guard, no trailing commas.
#define DC_VARIANT(BM, BN, BK, WR, WC, WK, PF) DC_ROW_F32(#BM "x" #BN "x" #BK "_w" #WR #WC #WK "_p" #PF, BM, BN, BK, WR, WC, WK, PF, 0, false, false)
#define DC_VARIANT_MC(BM, BN, BK, WR, WC, WK, PF) DC_ROW_F32(#BM "x" #BN "x" #BK "_w" #WR #WC #WK "_p" #PF, BM, BN, BK, WR, WC, WK, PF, 0, false, true)
#define DC_VARIANT_H(BM, BN, BK, WR, WC, WK, PF) DC_ROW_F16("h" #BM "x" #BN "x" #BK "_w" #WR #WC #WK "_p" #PF, BM, BN, BK, WR, WC, WK, PF, 0, false, false)
#define DC_VARIANT_H_MC(BM, BN, BK, WR, WC, WK, PF) DC_ROW_F16("h" #BM "x" #BN "x" #BK "_w" #WR #WC #WK "_p" #PF, BM, BN, BK, WR, WC, WK, PF, 0, false, true)
// LDS-DMA variants: "d" prefix, BK fixed by the 128-byte row (64 halves), S = LDS stages of the ring
#define DC_VARIANT_HD(BM, BN, WR, WC, WK, S) DC_ROW_F16("d" #BM "x" #BN "x64_w" #WR #WC #WK "_s" #S, BM, BN, 64, WR, WC, WK, 1, S, true, false)
#define DC_VARIANT_HD_T(BM, BN, WR, WC, WK, S) /* LDS-transposed epilogue instead of the swapped-operand one (A/B) */ \
  DC_ROW_F16("d" #BM "x" #BN "x64_w" #WR #WC #WK "_s" #S "_t", BM, BN, 64, WR, WC, WK, 1, S, false, false)
#define DC_VARIANT_HD_MC(BM, BN, WR, WC, WK, S) DC_ROW_F16("d" #BM "x" #BN "x64_w" #WR #WC #WK "_s" #S, BM, BN, 64, WR, WC, WK, 1, S, true, true)
#define DC_VARIANT_HD2(BM, BN, WR, WC, WK, S) /* 256-byte rows: BK = 128 halves */ \
  DC_ROW_F16("d" #BM "x" #BN "x128_w" #WR #WC #WK "_s" #S, BM, BN, 128, WR, WC, WK, 1, S, true, false)
#define DC_VARIANT_FD(BM, BN, BK, WR, WC, WK, S) /* float32: BK = 32 (128-byte rows) or 64 (256-byte rows) */ \
  DC_ROW_F32("e" #BM "x" #BN "x" #BK "_w" #WR #WC #WK "_s" #S, BM, BN, BK, WR, WC, WK, 1, S, true, false)
// bfloat16 (v_mfma_f32_32x32x16_bf16, fp32 accumulate): the float16 tiles again, "b" / "bd" for "h" / "d" — same bytes, same
// instruction rate, so the same shapes win; a table of its own (kBf16Variant0 + i), the float16 / float32 one keeps its indices
#define DC_VARIANT_B(BM, BN, BK, WR, WC, WK, PF) DC_ROW_BF16("b" #BM "x" #BN "x" #BK "_w" #WR #WC #WK "_p" #PF, BM, BN, BK, WR, WC, WK, PF, 0, false, false)
#define DC_VARIANT_B_MC(BM, BN, BK, WR, WC, WK, PF) DC_ROW_BF16("b" #BM "x" #BN "x" #BK "_w" #WR #WC #WK "_p" #PF, BM, BN, BK, WR, WC, WK, PF, 0, false, true)
#define DC_VARIANT_BD(BM, BN, WR, WC, WK, S) DC_ROW_BF16("bd" #BM "x" #BN "x64_w" #WR #WC #WK "_s" #S, BM, BN, 64, WR, WC, WK, 1, S, true, false)
#define DC_VARIANT_BD_T(BM, BN, WR, WC, WK, S) DC_ROW_BF16("bd" #BM "x" #BN "x64_w" #WR #WC #WK "_s" #S "_t", BM, BN, 64, WR, WC, WK, 1, S, false, false)
#define DC_VARIANT_BD_MC(BM, BN, WR, WC, WK, S) DC_ROW_BF16("bd" #BM "x" #BN "x64_w" #WR #WC #WK "_s" #S, BM, BN, 64, WR, WC, WK, 1, S, true, true)
#define DC_VARIANT_BD2(BM, BN, WR, WC, WK, S) DC_ROW_BF16("bd" #BM "x" #BN "x128_w" #WR #WC #WK "_s" #S, BM, BN, 128, WR, WC, WK, 1, S, true, false)

// ---- kVariants
DC_VARIANT(128, 128, 32, 2, 2, 1, 2)  // 0: big-M layers (res2/res3)
DC_VARIANT(128, 64, 32, 2, 2, 1, 2)   // 1
DC_VARIANT(64, 128, 32, 2, 2, 1, 2)   // 2
DC_VARIANT_MC(64, 64, 32, 2, 2, 1, 3) // 3
DC_VARIANT_MC(64, 64, 64, 2, 2, 1, 3) // 4
DC_VARIANT_MC(32, 64, 64, 1, 2, 2, 4) // 5: in-workgroup split-K 2
DC_VARIANT(64, 32, 64, 2, 1, 2, 4)    // 6
DC_VARIANT_MC(32, 32, 128, 1, 1, 4, 3) // 7: split-K 4 (tiny M*N, long K: res4/res5)
DC_VARIANT_MC(32, 32, 64, 1, 1, 4, 4) // 8: same for K segments that are only multiples of 64
DC_VARIANT(32, 64, 32, 1, 2, 2, 4)    // 9: K segments that are only multiples of 32 (the stem)
// 8-wave workgroups: two waves per SIMD, so one wave's LDS/global/SALU work hides under the other's MFMAs
DC_VARIANT_MC(32, 64, 64, 1, 2, 4, 4) // 10
DC_VARIANT_MC(64, 64, 64, 2, 2, 2, 3) // 11
DC_VARIANT_MC(128, 64, 32, 2, 2, 2, 2) // 12 (multi-class too: the merged heads fetch 8.7x their minimum on 32x32 tiles)
DC_VARIANT_MC(128, 128, 32, 2, 2, 2, 2) // 13
DC_VARIANT(64, 64, 32, 2, 2, 2, 3)    // 14
DC_VARIANT_MC(32, 32, 128, 1, 1, 8, 3) // 15
DC_VARIANT_MC(64, 128, 32, 2, 2, 2, 2) // 16
// fp16 operands (v_mfma_f32_32x32x16_f16, fp32 accumulate); BK in halves: 64 = one 128-B line per row
DC_VARIANT_H_MC(128, 128, 64, 2, 2, 1, 2)   // 17 (multi-class too: the float16 heads at batch 8 run 26 % faster on 128-wide tiles)
DC_VARIANT_H_MC(128, 64, 64, 2, 2, 1, 2)    // 18
DC_VARIANT_H(64, 128, 64, 2, 2, 1, 2)    // 19
DC_VARIANT_H_MC(64, 64, 64, 2, 2, 1, 3)  // 20
DC_VARIANT_H_MC(64, 64, 128, 2, 2, 2, 2) // 21: 8 waves
DC_VARIANT_H_MC(32, 64, 128, 1, 2, 2, 3) // 22
DC_VARIANT_H(64, 32, 128, 2, 1, 2, 3)    // 23
DC_VARIANT_H_MC(32, 64, 256, 1, 2, 4, 2) // 24: 8 waves, split-K 4
DC_VARIANT_H_MC(128, 128, 128, 2, 2, 2, 2)  // 25: 8 waves
DC_VARIANT_H_MC(32, 32, 256, 1, 1, 4, 2) // 26
// deeper rings for the short-K (bandwidth-class) layers: three of the four K tiles of a K = 256 layer are in flight at once
DC_VARIANT_H(128, 128, 64, 2, 2, 1, 3)   // 27
DC_VARIANT_H(128, 64, 64, 2, 2, 1, 3)    // 28
DC_VARIANT_H(64, 128, 64, 2, 2, 1, 3)    // 29
// 256-row / 256-column tiles (one workgroup per CU): half the operand traffic per flop for the long-K matrix-class layers
DC_VARIANT_H(256, 128, 64, 4, 2, 1, 2)   // 30
DC_VARIANT_H(128, 256, 64, 2, 4, 1, 2)   // 31
// float16 through LDS-DMA (round 3): no register ring, no ds_write, unpadded swizzled stages, swapped-operand epilogue.
// (Measured and dropped: 4 waves with a 3-stage ring on 128x128 — one workgroup per CU without a second wave per SIMD —,
//  256-byte rows on 128x128, the LDS-transposed epilogue on the 8-wave tile.)
DC_VARIANT_HD_MC(128, 128, 2, 2, 1, 2)   // 32: 66 KB -> two workgroups per CU
DC_VARIANT_HD_MC(128, 128, 2, 2, 2, 3)   // 33: 8 waves, 98 KB, two tiles ahead: the 196-workgroup res4 layers
DC_VARIANT_HD(128, 128, 2, 2, 2, 4)      // 34: 8 waves, 130 KB, three tiles ahead
DC_VARIANT_HD(128, 64, 2, 2, 1, 3)       // 35: 73 KB -> two per CU
DC_VARIANT_HD(64, 128, 2, 2, 1, 3)       // 36
DC_VARIANT_HD(64, 64, 2, 2, 1, 4)        // 37: 65 KB
DC_VARIANT_HD_MC(256, 128, 4, 2, 1, 3)   // 38: 146 KB, one per CU: the long-K matrix-class layers
DC_VARIANT_HD_MC(128, 256, 2, 4, 1, 3)   // 39
DC_VARIANT_HD(128, 64, 2, 2, 1, 2)       // 40: 49 KB -> three workgroups per CU (the bandwidth-class layers)
DC_VARIANT_HD(64, 128, 2, 2, 1, 2)       // 41
DC_VARIANT_HD(64, 64, 2, 2, 1, 2)        // 42: 33 KB
DC_VARIANT_HD2(64, 64, 2, 2, 2, 2)       // 43: 256-byte rows, 8 waves
DC_VARIANT_HD2(32, 64, 1, 2, 4, 3)       // 44: split-K 4 (small maps)
DC_VARIANT_HD_T(128, 128, 2, 2, 1, 2)    // 45: LDS-transposed epilogue instead of the swapped-operand one
DC_VARIANT_HD_T(64, 128, 2, 2, 1, 2)     // 46
// float32 through LDS-DMA: the fp32 matrix pipe is 16x slower than the fp16 one, staging is not its limiter — these
// tie with the register-ring tiles (+-3 % at batch 1, up to -5 % at batch 8: EXPERIMENTS.md A); the autotuner takes the wins
DC_VARIANT_FD(32, 64, 64, 1, 2, 4, 3)    // 47: the res4/res5 batch-1 tile (8 waves, split-K 4)
DC_VARIANT_FD(64, 128, 32, 2, 2, 2, 3)   // 48
DC_VARIANT_FD(64, 64, 32, 2, 2, 2, 4)    // 49
DC_VARIANT_FD(128, 64, 32, 2, 2, 2, 3)   // 50
DC_VARIANT_FD(32, 32, 64, 1, 1, 4, 4)    // 51
DC_VARIANT_FD(64, 64, 32, 2, 2, 1, 4)    // 52: 4 waves
// 8 waves on 128x128 WITHOUT the in-workgroup split-K (wave tile 32x64 / 64x32): no exchange through LDS before the epilogue
// (res4 3x3 21.5 -> 21.0 us, 1024->256 12.3 -> 11.7 at batch 8; bit-identical to the 4-wave tile's sums)
DC_VARIANT_HD(128, 128, 4, 2, 1, 3)      // 53
DC_VARIANT_HD(128, 128, 2, 4, 1, 3)      // 54

// ---- kVariantsBf16
DC_VARIANT_B_MC(128, 128, 64, 2, 2, 1, 2) // 0
DC_VARIANT_B_MC(128, 64, 64, 2, 2, 1, 2) // 1
DC_VARIANT_B(64, 128, 64, 2, 2, 1, 2)  // 2
DC_VARIANT_B_MC(64, 64, 64, 2, 2, 1, 3) // 3
DC_VARIANT_B_MC(64, 64, 128, 2, 2, 2, 2) // 4
DC_VARIANT_B_MC(32, 64, 128, 1, 2, 2, 3) // 5
DC_VARIANT_B(64, 32, 128, 2, 1, 2, 3)  // 6
DC_VARIANT_B_MC(32, 64, 256, 1, 2, 4, 2) // 7
DC_VARIANT_B_MC(128, 128, 128, 2, 2, 2, 2) // 8
DC_VARIANT_B_MC(32, 32, 256, 1, 1, 4, 2) // 9
DC_VARIANT_B(128, 128, 64, 2, 2, 1, 3) // 10
DC_VARIANT_B(128, 64, 64, 2, 2, 1, 3)  // 11
DC_VARIANT_B(64, 128, 64, 2, 2, 1, 3)  // 12
DC_VARIANT_B(256, 128, 64, 4, 2, 1, 2) // 13
DC_VARIANT_B(128, 256, 64, 2, 4, 1, 2) // 14
DC_VARIANT_BD_MC(128, 128, 2, 2, 1, 2) // 15
DC_VARIANT_BD_MC(128, 128, 2, 2, 2, 3) // 16
DC_VARIANT_BD(128, 128, 2, 2, 2, 4)    // 17
DC_VARIANT_BD(128, 64, 2, 2, 1, 3)     // 18
DC_VARIANT_BD(64, 128, 2, 2, 1, 3)     // 19
DC_VARIANT_BD(64, 64, 2, 2, 1, 4)      // 20
DC_VARIANT_BD_MC(256, 128, 4, 2, 1, 3) // 21
DC_VARIANT_BD_MC(128, 256, 2, 4, 1, 3) // 22
DC_VARIANT_BD(128, 64, 2, 2, 1, 2)     // 23
DC_VARIANT_BD(64, 128, 2, 2, 1, 2)     // 24
DC_VARIANT_BD(64, 64, 2, 2, 1, 2)      // 25
DC_VARIANT_BD2(64, 64, 2, 2, 2, 2)     // 26
DC_VARIANT_BD2(32, 64, 1, 2, 4, 3)     // 27
DC_VARIANT_BD_T(128, 128, 2, 2, 1, 2)  // 28
DC_VARIANT_BD_T(64, 128, 2, 2, 1, 2)   // 29
DC_VARIANT_BD(128, 128, 4, 2, 1, 3)    // 30
DC_VARIANT_BD(128, 128, 2, 4, 1, 3)    // 31

#undef DC_ROW_F32
#undef DC_ROW_F16
#undef DC_ROW_BF16
