/*
 * mxdet_debug.h -- tuning and test hooks of libmxdet_hip.so. NOT part of the drop-in boundary (include/mxdet.h):
 * nothing a reference-side binding calls is declared here. Unlike the boundary's entries, the hooks set state that
 * later calls read (per calling thread where noted, otherwise library-wide): sweeps and tests only.
 */
#ifndef MXDET_DEBUG_H_
#define MXDET_DEBUG_H_

#include <stdint.h>

#include "mxdet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* force the conv tile configuration on this thread (0 = built-in heuristic, else a case of conv.hip launch()) */
int mxdet_debug_force_conv_cfg(int32_t cfg);
/* force the split-K factor of mxdet_conv2d_wgrad on the calling thread (0 = heuristic) */
int mxdet_debug_force_wgrad_ksplit(int32_t ksplit);
/* 1 = always use the direct-gather preprocess kernel (the wide-frame path); library-wide */
int mxdet_debug_preprocess_direct(int32_t on);

/* Plan-time thresholds of the tile / split heuristics (library-wide; value < 0 restores the built-in default).
 * The library itself never reads the environment: tools that sweep these call the hook. */
#define MXDET_TUNE_T64 0          /* conv: 64-row tiles from this many tiles on (default 400) */
#define MXDET_TUNE_T128 1         /* conv: 256x256 (+ tail) tiles from this many 128x128 tiles on (default 1536) */
#define MXDET_TUNE_PAR64 2        /* stride-2 dgrad: 64x128 tiles from this many tiles on (default 1600) */
#define MXDET_TUNE_WG_TARGET 3    /* grouped wgrad: workgroups per group aimed for (default 3072) */
#define MXDET_TUNE_WG_MINSTEPS 4  /* grouped wgrad: fewest 32-pixel steps per workgroup (default 64) */
#define MXDET_TUNE_WG_MAXSTEPS 5  /* grouped wgrad: most steps per workgroup (default 128) */
#define MXDET_TUNE_T3_ENABLE 6    /* wgrad: 1 = 3x3 / stride 1 / pad 1 layers use the three-tap tile (wgrad3_tile.h; default 1) */
#define MXDET_TUNE_T3_TARGET 7    /* ... workgroups of that kernel per group aimed for (default 1536) */
#define MXDET_TUNE_T3_MINSTEPS 8  /* ... fewest 64-pixel steps per workgroup (default 32: neutral for the two large groups of the single-GPU step, +1.9 % for the five smaller ones of the exchange schedule) */
#define MXDET_TUNE_T3_NS 9        /* ... LDS-DMA ring depth, 2 or 3 (default 2) */
#define MXDET_TUNE_TAIL 10        /* conv: tiles of the rows left over by the 256x256 rounds: 0 = 128x128, 1 = 64x128, 2 = 64x64 */
#define MXDET_TUNE_WG_NS 11       /* grouped wgrad (128x128 tiles): LDS-DMA ring depth 2, 3 or 4 */
#define MXDET_TUNE_ROI_TABLE 12   /* RoIAlign backward (gather): 1 = the three-kernel table form instead of the segment form */
#define MXDET_TUNE_ROI_ROWS 13    /* RoIAlign backward, segment form: rows per tile on maps with >= 64 rows (default 2) */
#define MXDET_TUNE_STATIC_TAPS 14 /* conv: 1 = stride-1 1x1 / 3x3 layers use the unrolled static-tap K loop (default 1) */
#define MXDET_TUNE_T128W 15     /* conv: stride-1 1x1 / 3x3 layers of >= 128 columns use 128x128 tiles of eight waves from this many
                                    128x128 tiles on (default 1000000 = never; measured in profiles/r02_d_static_cfg_sweep.txt) */
#define MXDET_TUNE_T3_MIX 16    /* grouped wgrad: three-tap and one-tap tiles in ONE grid (0 = two launches; 1 = one-tap ring of 3
                                    stages inside the three-tap kernel's LDS; 2 = ring of 2; default 1) */
#define MXDET_TUNE_SPLITK_TILE 17 /* mxdet_conv2d_fwd_splitk: 0 = 64x64 tiles, 1 = 128x128 (four waves), 2 = 128x128 (eight waves) */
#define MXDET_TUNE_T3_PER_ITEM 18  /* grouped wgrad, three-tap tiles: at most this many workgroups per 3x3 layer of the group (0 = no cap; default 192) */
#define MXDET_TUNE_COUNT 19
int mxdet_debug_set_tuning(int32_t which, int64_t value);
/* the value in effect (tests check that what they changed is back); -1 and an error string for an unknown key */
int64_t mxdet_debug_get_tuning(int32_t which);


/* Route probe (per calling thread): which kernel instantiation a dense convolution / weight-gradient call, or which
 * form of the RetinaNet level loss, runs.
 * While the probe is on, mxdet_conv2d_fwd / _fwd_splitk / _fwd_chain / _dgrad / _grouped, mxdet_conv2d_wgrad,
 * mxdet_conv2d_wgrad_grouped(_parts), mxdet_retina_loss_level(_iou / _quality / _dfl / _ghm) and mxdet_ghm_hist_level validate
 * their arguments as usual, record the launch(es) they WOULD make and return
 * MXDET_OK without launching, without dereferencing any pointer and without touching the device (so it also works on a
 * machine without a GPU, with dummy non-null pointers). Switching it on clears the records. A record is 16 int32 words,
 * word 0 = kind:
 *   MXDET_ROUTE_CONV          BM, BN, WM, WN, NS, DGRAD, PAR, TAPS, CHAIN, tiles_m, tiles_n, m_begin, ksplit, grid
 *                             (one per kernel launch: a 256x256 launch and its tail are two records)
 *   MXDET_ROUTE_WGRAD         three-tap (0/1), ksplit, steps_per_split, t3_steps, ring depth of the three-tap kernel (0 = not
 *                             launched), ring depth of the one-tap kernel (0 = not launched), fold (0/1), one-tap grid (tiles +
 *                             bias workgroups), three-tap grid, accumulate, one-tap steps (of MXDET_WGRAD_BKP pixels), three-tap
 *                             steps (of 64 virtual pixels)
 *   MXDET_ROUTE_CONV_GROUPED  BM, BN, WM, WN, NS, DGRAD, 0, TAPS, 0, 0, 0, 0, 0, grid, items
 *   MXDET_ROUTE_WGRAD_GROUPED mixed grid (0 / 1 / 2 = MXDET_TUNE_T3_MIX in effect), ring depth three-tap tiles, ring depth
 *                             one-tap tiles (0 = none launched), grid_big, grid_wgrad, grid_reduce (after `parts`), parts
 *   MXDET_ROUTE_RETINA_LOSS   vec (1 = the 16-byte form retina_loss_kernel<true>, 0 = the scalar form: C, ld_cls or ld_reg not
 *                             a multiple of 8 / 8 / 4, or cls / grad_cls not 16-byte or reg / grad_reg not 8-byte aligned),
 *                             grid (= mxdet_retina_loss_num_partials)
 *   MXDET_ROUTE_RETINA_LOSS_IOU  the same two words for mxdet_retina_loss_level_iou (retina_loss_iou_kernel<vec, false>)
 *   MXDET_ROUTE_RETINA_LOSS_QUALITY  the same two words for mxdet_retina_loss_level_quality (retina_loss_iou_kernel<vec, true>)
 *   MXDET_ROUTE_RETINA_LOSS_DFL  the same two words for mxdet_retina_loss_level_dfl (retina_loss_dfl_kernel<vec, focal>)
 *   MXDET_ROUTE_RETINA_LOSS_GHM  the same two words for mxdet_retina_loss_level_ghm (retina_loss_ghm_kernel<vec, cls, reg>),
 *                             then flags (MXDET_GHM_CLS | MXDET_GHM_REG)
 *   MXDET_ROUTE_GHM_HIST      the same three words for mxdet_ghm_hist_level (ghm_hist_kernel<vec>). mxdet_ghm_weights has one
 *                             route: while the probe is on it validates its arguments and returns MXDET_OK without a launch
 *                             and without a record, so the head's whole sequence can be probed on a machine without a GPU */
#define MXDET_ROUTE_CONV 1
#define MXDET_ROUTE_WGRAD 2
#define MXDET_ROUTE_CONV_GROUPED 3
#define MXDET_ROUTE_WGRAD_GROUPED 4
#define MXDET_ROUTE_RETINA_LOSS 5
#define MXDET_ROUTE_RETINA_LOSS_IOU 6
#define MXDET_ROUTE_RETINA_LOSS_QUALITY 7
#define MXDET_ROUTE_RETINA_LOSS_DFL 8
#define MXDET_ROUTE_RETINA_LOSS_GHM 9
#define MXDET_ROUTE_GHM_HIST 10
#define MXDET_ROUTE_WORDS 16
#define MXDET_ROUTE_MAX 4
int mxdet_debug_route_probe(int32_t on);
/* copies up to max_records (<= MXDET_ROUTE_MAX) records to `records` ([max_records][16]); returns the number of launches
 * recorded since the probe was switched on (more than MXDET_ROUTE_MAX are counted but not kept) */
int mxdet_debug_route_read(int32_t* records, int32_t max_records);

/* Which route mxdet_group_norm_fwd / _bwd take for this descriptor (a pure function of HW and C; no device access):
 * MXDET_GN_ROUTE_RESIDENT or MXDET_GN_ROUTE_TILED, or the negative code the entry itself would return for the shape. */
#define MXDET_GN_ROUTE_RESIDENT 1
#define MXDET_GN_ROUTE_TILED 2
int mxdet_debug_group_norm_route(const mxdet_gn_desc_t* d);

#ifdef __cplusplus
}
#endif
#endif /* MXDET_DEBUG_H_ */
