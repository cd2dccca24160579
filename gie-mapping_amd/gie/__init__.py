"""gie — host-side Python mirror of the GIE-mapping per-frame update over the MI355X C-ABI."""
from ._capi import CamParam, CloudParam, CloudPoint, Config, CostMapHdr, FrameStats, FrontierCluster, FrontierParam, GroundCell, GroundNf1Param, GroundParam, LosHit, LosParam, MultiScanParam, ScanParam, ShortcutInfo, ShortcutParam, View, ViewParam, ViewScore, Voxel, Waypoint  # noqa: F401
from .mapper import (CLOUD_DIST, CLOUD_DTYPE, CLOUD_NO_BAND, CLOUD_TYPE, VOX_FNT, VOX_FREE, VOX_OCCUPIED, VOX_UNKNOWN, FRONTIER_CLUSTER_DTYPE, GROUND_CELL_DTYPE, GROUND_NF1_FROM_FRONTIERS, GROUND_NF1_UNKNOWN_TRAVERSABLE, GROUND_UNKNOWN_BLOCKS, LIB_PATH, LOS_HIT_DTYPE, LOS_UNKNOWN_OPAQUE, SHORTCUT_INFO_DTYPE, VIEW_DTYPE, VIEW_SCORE_DTYPE, WAYPOINT_DTYPE, Mapper, MapperBase,
                     flt2grids_sq, load_library, make_config, make_views, view_frustum)  # noqa: F401
from . import scenes, tiling  # noqa: F401
