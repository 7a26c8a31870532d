/*
 * grandplus_order.h -- the internal entry points behind option "row_order" (implemented by grand_plus_amd/csrc/gfpush.hip).
 *
 * Part of the ABI that grandplus.h describes (gp_graph and the status codes are defined there): grandplus.h includes this
 * file, so callers include grandplus.h alone.  The ctypes binding declares the entry points under this file's name in
 * _native.ABI, and tests/test_host_abi.py holds that table against this file type by type.
 */
#ifndef GRANDPLUS_ORDER_H
#define GRANDPLUS_ORDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* internal (tests): the order in which the first launch of g's last gp_gfpush_device call handed out its rows (option
 * "row_order" = 1: heaviest first, by the cost class grand_plus_amd/row_cost.py restates).  Waits for that call.  *n_rows =
 * rows of that call, or 0 when it ran in caller order (row_order = 0, or no more rows than workgroups); h_order (NULL: sizes
 * only) takes that many row numbers, a permutation of 0 .. *n_rows - 1, and must have room for `cap` >= *n_rows of them.
 * *deg_shift / *deg_sat: the degree field of the column words the cost was read from (word >> shift, saturating at sat). */
int gp_internal_row_order(gp_graph* g, uint32_t* h_order, int64_t cap, int64_t* n_rows, int* deg_shift, uint32_t* deg_sat);

/* internal (tools/sk_phases.py): per workgroup of the last sketch-kernel launch { stamp at entry, stamp at leaving the row loop }
 * on the constant 100 MHz clock, 2 * n_workgroups values (n_workgroups <= 65 536).  Kept by the -DGP_SK_TIMING build only:
 * all 0 in the product library. */
int gp_internal_wg_log(gp_graph* g, int64_t* out, int n_workgroups);

#ifdef __cplusplus
}
#endif
#endif /* GRANDPLUS_ORDER_H */
