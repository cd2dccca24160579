/*
 * edt_plan_probe.cpp — TEST-ONLY: the product's gie_edt_plan_for (gie_edt_plan.h; which kernels the batch EDT launches, with which
 * template arguments, grids and scalar arguments) compiled for the host, its fields as integers (tests/test_edt_plan_host.py).
 */
#include "../../gie-mapping_amd/csrc/gie_edt_plan.h"

/* the names of out[]'s fields, comma separated, in order */
extern "C" const char *gie_probe_edt_plan_fields(void)
{
    return "y_kernel,y_grid,y_block_x,y_block_y,cp_x,cp_z,zs,guess,x,x_zs,x_grid_x,x_grid_y,stream,stream_fused,nseg,seg_len,stream_grid,"
           "stream_note,direct,direct_grid,redo,redo_grid,col_lds,col_grid,col_ntx,col_ntiles";
}
extern "C" void gie_probe_edt_plan(int X, int Y, int Z, int cu_total, int full, int guess, int completion, int zs_fused_switch, int32_t *out)
{
    const gie_edt_plan p = gie_edt_plan_for(X, Y, Z, cu_total, full, guess, completion, zs_fused_switch);
    const int v[] = { p.y_kernel, p.y_grid, p.y_block[0], p.y_block[1], p.cp_x, p.cp_z, p.zs, p.guess, p.x, p.x_zs, p.x_grid[0], p.x_grid[1],
                      p.stream, p.stream_fused, p.nseg, p.seg_len, p.stream_grid, p.stream_note, p.direct, p.direct_grid, p.redo, p.redo_grid,
                      p.col_lds, p.col_grid, p.col_ntx, p.col_ntiles };
    for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); i++) out[i] = v[i];
}
/* the launch constants and enumerators the test restates */
extern "C" void gie_probe_edt_plan_consts(int32_t *out)
{
    const int v[] = { GIE_EDT_Y_NONE, GIE_EDT_Y4_16, GIE_EDT_Y4_32, GIE_EDT_Y_8_8, GIE_EDT_Y_16_16, GIE_EDT_Y_32_16,
                      GIE_EDT_HINT_NONE, GIE_EDT_HINT_LEFT, GIE_EDT_HINT_TOOK,
                      GIE_EDTY_COLS, GIE_EDTY4_LANES, GIE_EDTX_WAVES, GIE_ZSTREAM_WAVES, GIE_EDTZ_TX, GIE_EDTZ_WAVES, GIE_LDS_BYTES };
    for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); i++) out[i] = v[i];
}
