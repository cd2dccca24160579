/*
 * edty_strip_probe.cpp — TEST-ONLY: the product's gie_edty_strip / gie_edty_groups (gie_ops.h; which (strip, z) a workgroup of EDT
 * pass Y takes) compiled for the host, one call per linear workgroup index of a launch (tests/test_edty_strip_host.py).
 */
#include "gie_platform_emu.h"
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <cmath>
#include "../../gie-mapping_amd/csrc/gie_functors.h"

/* the launch's number of workgroups */
extern "C" int gie_probe_edty_grid(int nstrip, int Z) { return 16 * gie_edty_groups(nstrip, Z); }
/* out[3 l .. 3 l + 2] = (valid, strip, z) of linear index l, for every l of the launch */
extern "C" void gie_probe_edty_strip(int nstrip, int Z, int32_t *out)
{
    const int n = 16 * gie_edty_groups(nstrip, Z);
    for (int l = 0; l < n; l++) {
        int strip = -1, z = -1;
        out[3 * l] = gie_edty_strip(l, nstrip, Z, &strip, &z);
        out[3 * l + 1] = strip; out[3 * l + 2] = z;
    }
}
