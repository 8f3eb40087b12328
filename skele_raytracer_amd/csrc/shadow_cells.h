// Shape of the per-light shadow masks, shared by the host builder (scene_masks.cpp build_shadow_masks) and the device lookup
// (shade_common.h shadow_mask_of).  DESIGN.md "Shadow masks" has the derivation of the margins.
#pragma once

#include <stdint.h>

/* Cells per edge of one cube face: a light's table has 6 x N x N cells of one uint32_t each (N = 32: 6144 cells, 24 KB).  Cell
 * (face, i, j) of a direction v: the face is the axis of v's largest |component| (ties: x before y before z) and its sign,
 * face = 2 axis + (v[axis] < 0); (i, j) = the cells of v's other two components in axis order, divided by |v[axis]|, on
 * [-1, 1] cut into N equal parts (clamped).  Bit k of a cell: sphere k may stop a shadow ray of that light whose direction
 * lies in the cell. */
#ifndef SKR_SHADOW_CELLS
#define SKR_SHADOW_CELLS 32
#endif
#define SKR_SHADOW_TABLE_WORDS (6 * SKR_SHADOW_CELLS * SKR_SHADOW_CELLS) /* per light */
#define SKR_SHADOW_MAX_SPHERES 32 /* one bit per sphere; more spheres keep the plain loop */

/* Surface patches of the shadow masks (DESIGN.md "Shadow surface patches"): a shading point P that is a hit of sphere s is keyed to
 * the cell of e = P - C_s in a cube map of G_s x G_s cells per face on that sphere (the addressing above), where the device's
 * fl(|e|^2) - r_s^2 is within the radial slack tau_s = r_s^2 * SKR_SURFACE_SLACK.  One table per pair of lights (2p, 2p + 1), `stride`
 * words each; word base_s + (f G_s + i) G_s + j of a pair's table = the union over the pair's lights of the spheres that may be
 * candidates of a shadow ray from any point of that patch.  The header of sphere s is one word, base_s | G_s << 24 (G_s = 0: no
 * patches), kept in the .w of the sphere's kd row, which travels to LDS with the staged scene. */
#define SKR_SURFACE_SLACK 0x1p-7f
#ifndef SKR_SHADOW_SURFACE_SCALE
#define SKR_SHADOW_SURFACE_SCALE 4 /* cells per edge of a GI surface patch's cell (SKR_GI_SURFACE_MAX_CELLS caps G_s here too); 1, 2, 4 measured: DESIGN.md */
#endif
#define SKR_SHADOW_SURFACE_MAX_BYTES (1u << 20) /* every pair's table together */

/* GI masks (DESIGN.md "GI masks"): the node pipeline's closest-hit walk of a GI child ray visits only the spheres named by the mask
 * of (the cell of its origin, the cell of its direction).  Origins are looked up in a fine grid over the small spheres, then in a
 * coarse grid around it (SkrGiGrid: cubic cells, cell (i, j, k) of a point o = the integer parts of (o - lo) * inv, each in [0, n);
 * index[base + (k n1 + j) n0 + i] = the cell's row of masks, -1 = none).  A row holds the masks of 6 x G x G direction cells, G =
 * SKR_GI_DIR_CELLS, addressed like a light's shadow table; uint16_t masks where the scene has at most 16 spheres, else uint32_t.
 * Bit k: a ray from any origin of the cell along any direction of the direction cell may have D >= 0 and b < 0 for sphere k. */
#ifndef SKR_GI_DIR_CELLS
#define SKR_GI_DIR_CELLS 16
#endif
#define SKR_GI_ROW_ENTRIES (6 * SKR_GI_DIR_CELLS * SKR_GI_DIR_CELLS) /* masks per origin cell */
#define SKR_GI_MAX_SPHERES 32
#define SKR_GI_MAX_BYTES (2u << 20) /* the whole table (index and masks): small enough to stay in L2 */
struct SkrGiGrid {
	float lo[3], inv; /* lo: the grid's corner; inv: 1 / the cell's edge */
	float n_f[3];     /* n as floats (the device's range test) */
	int32_t n[3], base;
};

/* Surface patches of the GI masks (DESIGN.md "GI surface patches"): a GI origin is a hit point of sphere s, so its row can be keyed
 * to the cell of e = o - C_s in a cube map of G_s x G_s cells per face on that sphere (the addressing above, G_s per sphere), where
 * the device's fl(|e|^2) - r_s^2 is within the sphere's radial slack tau_s.  Per sphere SKR_GI_SURFACE_HEAD words: the first index
 * word (from the start of the headers), G_s, tau_s (binary32 bits; negative: no patches), 0.  Index word (f G_s + i) G_s + j = the
 * patch's row of masks (numbered after the grids' rows), -1 = none. */
#define SKR_GI_SURFACE_HEAD 4
#define SKR_GI_SURFACE_MAX_CELLS 128 /* G_s at most: the ground-like spheres' index stays small */
