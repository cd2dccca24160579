/*
 * block_observed_probe.cpp — TEST-ONLY: the product's gie_block_observed (gie_ops.h; the question k_cell_alloc asks of a label plane
 * left in place) compiled for the host, one call per table cell (tests/test_block_observed_host.py).
 */
#include "gie_platform_emu.h"
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <cmath>
#include "../../gie-mapping_amd/csrc/gie_functors.h"

/* out[cell] = gie_block_observed for every cell of a table of tdim cells whose first block is tb0; the plane is size[0] x size[1] x size[2] bytes at `labels` */
extern "C" void gie_probe_block_observed(const int8_t *labels, const int32_t *size, const int32_t *pvt, const int32_t *tb0, const int32_t *tdim, uint8_t *out)
{
    static gie_ctx c;                                     /* (zero: the helper reads the sizes, the pivot and the table origin only) */
    c.X = size[0]; c.Y = size[1]; c.Z = size[2];
    for (int i = 0; i < 3; i++) { c.pvt[i] = pvt[i]; c.tb0[i] = tb0[i]; c.tdim[i] = tdim[i]; }
    for (int bz = 0; bz < tdim[2]; bz++) for (int by = 0; by < tdim[1]; by++) for (int bx = 0; bx < tdim[0]; bx++)
        out[(bz * tdim[1] + by) * tdim[0] + bx] = (uint8_t)gie_block_observed(c, labels, bx, by, bz);
}
