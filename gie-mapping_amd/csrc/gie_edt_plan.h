/*
 * gie_edt_plan.h — the batch EDT's launches as ONE statement: which kernels an update (be_edt) or the completion of a partial pass
 * (be_edt_z) launches, with which template arguments, grids and scalar arguments.  Integer arithmetic, no HIP type: gie_hip.hip executes
 * the plan and decides nothing, tests/emu/edt_plan_probe.cpp compiles it for the host.  What the DEVICE decides (gie_zs_takes) is not here.
 */
#ifndef GIE_EDT_PLAN_H
#define GIE_EDT_PLAN_H
#include <stddef.h>
#include "gie_types.h"
enum { GIE_EDT_Y_NONE = 0, GIE_EDT_Y4_16, GIE_EDT_Y4_32, GIE_EDT_Y_8_8, GIE_EDT_Y_16_16, GIE_EDT_Y_32_16 };   /* k_edt_y4<16> ... k_edt_y<32, 16> */
typedef struct gie_edt_plan {
    int y_kernel, y_grid, y_block[2];   /* GIE_EDT_Y_* (NONE: a completion); a linear grid: the kernels derive (strip, z) from the workgroup index (gie_edty_strip) */
    int cp_x, cp_z;                     /* the CP instantiation of a row / a column: 1, 2, 4, 8, 16 */
    int zs;                             /* the host half of gie_zs_takes: 0 = the streaming form never takes the volume, 1 = it reads pass X's planes, 2 = the fused form, which reads pass Y's */
    int guess;                          /* GIE_EDT_HINT_*, where it counts */
    int x, x_zs, x_grid[2];             /* k_edt_x<cp_x>: launched, its `zs` argument */
    int stream, stream_fused, nseg, seg_len, stream_grid, stream_note;   /* k_edt_z_stream<stream_fused>; note: it is told the guess and given the hint word */
    int direct, direct_grid;            /* k_edt_z_direct: the list form in a launch of its own */
    int redo, redo_grid;                /* k_edt_x_redo<cp_x>: pass X on the rows of the slabs the fused form gave up */
    int col_lds, col_grid, col_ntx, col_ntiles;   /* k_edt_z<cp_z, GIE_EDTZ_TX, GIE_EDTZ_WAVES> (always): dynamic LDS bytes, grid, tile counts */
} gie_edt_plan;
GIE_HD int gie_edt_cp(int L) { return L <= 64 ? 1 : L <= 128 ? 2 : L <= 256 ? 4 : L <= 512 ? 8 : 16; }
/* zs before the guess: short columns are the column kernel's; the fused form loads two columns to a dword (X even); fused_switch = GIE_ZS_FUSED */
GIE_HD int gie_edt_zs_host(int X, int Z, int fused_switch) { return (Z < 64 || Z > 1024) ? 0 : (fused_switch && (X & 1) == 0) ? 2 : 1; }
/* full = 1: pass Z over the whole volume; 0: only where Mark reads (the list form and the column kernel are both launched, the one the
 * known-tile count does not call for returns at once).  completion: pass Z again — pass Y is complete, pass X where the streaming form
 * does not take the volume.  Where the fused form may take the volume (zs 2) the device decides whether it does, and a launch made for
 * the other outcome costs its full time on the stream: pass X's 64 K workgroups that leave at once, or an empty k_edt_x_redo.  The
 * outcome barely moves from one update to the next, so an update is launched for the last one's (guess):
 *   TOOK: no pass X.  Should the form not take this volume after all, its kernel says so (GIE_CNT_XMISS) and the launches behind it do all of pass X and pass Z;
 *   LEFT: zs 1 — pass X in full, the streaming form from pass X's planes (which still takes the volume if this update's planes call for it), no k_edt_x_redo;
 *   NONE: both.  Exact whatever the guess: a wrong one costs time on that update only. */
GIE_HD gie_edt_plan gie_edt_plan_for(int X, int Y, int Z, int cu_total, int full, int guess, int completion, int zs_fused_switch)
{
    gie_edt_plan p;
    p.cp_x = gie_edt_cp(X); p.cp_z = gie_edt_cp(Z); p.zs = gie_edt_zs_host(X, Z, zs_fused_switch);
    p.guess = (p.zs == 2 && !completion) ? guess : GIE_EDT_HINT_NONE;
    if (p.guess == GIE_EDT_HINT_LEFT) p.zs = 1;
    /* pass Y: one 32-voxel mask word per thread (with only the planes that hold obstacles at work the pass is bound by how many loads are
     * in flight, not by bytes).  X % 4 == 0: four columns per lane, dword loads / 8-byte stores (k_edt_y4), 16 lanes per workgroup */
    const int y4 = (X & 3) == 0, yb = Y > 512 ? 32 : 16;
    p.y_kernel = completion ? GIE_EDT_Y_NONE : y4 ? (yb == 16 ? GIE_EDT_Y4_16 : GIE_EDT_Y4_32) : Y <= 256 ? GIE_EDT_Y_8_8 : Y <= 512 ? GIE_EDT_Y_16_16 : GIE_EDT_Y_32_16;
    p.y_grid = 16 * gie_edty_groups(y4 ? (X / 4 + GIE_EDTY4_LANES - 1) / GIE_EDTY4_LANES : (X + GIE_EDTY_COLS - 1) / GIE_EDTY_COLS, Z);
    p.y_block[0] = y4 ? GIE_EDTY4_LANES : GIE_EDTY_COLS; p.y_block[1] = y4 ? (Y + yb - 1) / yb : Y <= 256 ? 8 : 16;
    p.x = !completion && p.guess != GIE_EDT_HINT_TOOK; p.x_zs = p.zs == 2 ? 2 : 0;
    p.x_grid[0] = (Y + GIE_EDTX_WAVES - 1) / GIE_EDTX_WAVES; p.x_grid[1] = Z;
    /* the streaming form: a wave per (64 columns, y, z segment); z segments so that the launch has about eight waves per SIMD
     * (GIE_ZSTREAM_WAVES) to overlap its rows' round trips (a segment re-reads 16 planes).  The launch also carries the list form of the
     * pass (k_edt_z_direct's body) when `full` is 0: at least that kernel's grid */
    p.stream = p.zs != 0; p.stream_fused = p.zs == 2; p.stream_note = !completion;
    const int nxr = (X + 63) / 64, maxseg = Z / 64 > 0 ? Z / 64 : 1;
    int nseg = (int)(((long long)cu_total * 4 * GIE_ZSTREAM_WAVES + (long long)nxr * Y - 1) / ((long long)nxr * Y));
    nseg = nseg > maxseg ? maxseg : nseg < 1 ? 1 : nseg;
    p.seg_len = ((Z + nseg - 1) / nseg + 31) & ~31; p.nseg = (Z + p.seg_len - 1) / p.seg_len;
    long long grid = ((long long)nxr * p.nseg * Y + 3) / 4;
    if (grid > (long long)cu_total * 8 * 4) grid = (long long)cu_total * 8 * 4;
    p.direct_grid = cu_total * 16;
    if (!full && grid < p.direct_grid) grid = p.direct_grid;
    p.stream_grid = (int)grid; p.direct = p.zs == 0 && !full && !completion; p.redo = p.zs == 2; p.redo_grid = cu_total * 8;
    /* the column kernel (the rest, or the repair of the slabs the streaming form gave up): column tile + per-wave sites + plane list in
     * LDS, as many workgroups as fit one CU's (2 overlap load / envelope / store phases), tiles taken in pairs */
    const size_t LP = 64 * (size_t)p.cp_z, tile = ((size_t)Z * (GIE_EDTZ_TX + 1) + 3) & ~(size_t)3, lds = tile * 4 + GIE_EDTZ_WAVES * LP * 8 + LP * 2 + 16;
    p.col_lds = (int)lds; p.col_ntx = (X + GIE_EDTZ_TX - 1) / GIE_EDTZ_TX; p.col_ntiles = p.col_ntx * Y;
    int wgs = (int)(GIE_LDS_BYTES / (lds + 256));
    wgs = wgs < 1 ? 1 : wgs > 4 ? 4 : wgs;
    p.col_grid = wgs * cu_total < (p.col_ntiles + 1) / 2 ? wgs * cu_total : (p.col_ntiles + 1) / 2;
    return p;
}
#endif /* GIE_EDT_PLAN_H */
