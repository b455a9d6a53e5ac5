/* Prints the layout of the argument structs of include/kgx.h as a C11 compiler
 * sees them: one line `struct <name> <sizeof>`, then one line
 * `<field> <offsetof> <sizeof>` per field in declaration order.
 * tests/test_abi_layout_host.py compares it with the ctypes mirrors. */
#include <stddef.h>
#include <stdio.h>

#include "kgx.h"

#define STRUCT(T) printf("struct %s %zu\n", #T, sizeof(T))
#define FIELD(T, f) printf("%s %zu %zu\n", #f, offsetof(T, f), sizeof(((T*)0)->f))

int main(void) {
  STRUCT(kgx_work);
  FIELD(kgx_work, rowptr); FIELD(kgx_work, rows); FIELD(kgx_work, n_rows);
  FIELD(kgx_work, items); FIELD(kgx_work, n_items); FIELD(kgx_work, n_long_items); FIELD(kgx_work, n_short_end);
  FIELD(kgx_work, tiny_pack); FIELD(kgx_work, tiny_w); FIELD(kgx_work, n_tiny_deg2);
  FIELD(kgx_work, split); FIELD(kgx_work, n_split);
  FIELD(kgx_work, idx); FIELD(kgx_work, w);

  STRUCT(kgx_slice);
  FIELD(kgx_slice, items); FIELD(kgx_slice, lists); FIELD(kgx_slice, n_classes); FIELD(kgx_slice, tiles);
  FIELD(kgx_slice, idx); FIELD(kgx_slice, w); FIELD(kgx_slice, split); FIELD(kgx_slice, n_split);
  FIELD(kgx_slice, head_short_end);

  STRUCT(kgx_spmm_args);
  FIELD(kgx_spmm_args, struct_size);
  FIELD(kgx_spmm_args, reduce); FIELD(kgx_spmm_args, epilogue);
  FIELD(kgx_spmm_args, work);
  FIELD(kgx_spmm_args, table); FIELD(kgx_spmm_args, ld_table); FIELD(kgx_spmm_args, table2);
  FIELD(kgx_spmm_args, n_table1); FIELD(kgx_spmm_args, F);
  FIELD(kgx_spmm_args, out); FIELD(kgx_spmm_args, ld_out);
  FIELD(kgx_spmm_args, bias); FIELD(kgx_spmm_args, xroot); FIELD(kgx_spmm_args, ld_x);
  FIELD(kgx_spmm_args, gin_scale); FIELD(kgx_spmm_args, drop_p);
  FIELD(kgx_spmm_args, drop_key); FIELD(kgx_spmm_args, drop_seed);
  FIELD(kgx_spmm_args, partials); FIELD(kgx_spmm_args, counters);

  STRUCT(kgx_fused_args);
  FIELD(kgx_fused_args, struct_size);
  FIELD(kgx_fused_args, reduce); FIELD(kgx_fused_args, flags);
  FIELD(kgx_fused_args, work);
  FIELD(kgx_fused_args, x); FIELD(kgx_fused_args, ld_x); FIELD(kgx_fused_args, x2); FIELD(kgx_fused_args, n_x1);
  FIELD(kgx_fused_args, F_in);
  FIELD(kgx_fused_args, W); FIELD(kgx_fused_args, F_out); FIELD(kgx_fused_args, bias);
  FIELD(kgx_fused_args, gin_scale); FIELD(kgx_fused_args, pad_);
  FIELD(kgx_fused_args, out); FIELD(kgx_fused_args, ld_out); FIELD(kgx_fused_args, partials);
  FIELD(kgx_fused_args, agg_out); FIELD(kgx_fused_args, ld_agg);
  FIELD(kgx_fused_args, slice);
  return 0;
}
