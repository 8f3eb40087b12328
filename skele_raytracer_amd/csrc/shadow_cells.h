// Shape of the per-light shadow masks, shared by the host builder (scene_host.cpp build_shadow_masks) and the device lookup
// (shade_common.h shadow_mask_of).  DESIGN.md "Shadow masks" has the derivation of the margins.
#pragma once

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
