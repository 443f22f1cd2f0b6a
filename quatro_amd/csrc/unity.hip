// unity.hip — single translation unit of libquatro_hip.so (all kernels + the C ABI) and, with -DQTR_EXT_LIB and
// exports_ext.map, of libquatro_ext.so, with -DQTR_EXT2_LIB and exports_ext2.map, of libquatro_ext2.so, and, with
// -DQTR_EXT3_LIB and exports_ext3.map, of libquatro_ext3.so: the same code with the entry points of one group of extension
// headers visible.
#ifndef QTR_EXT_LIB  // libquatro_hip.so carries the extension code (its handle frees the maps) but exports none of it
#define QTR_EXT_API __attribute__((visibility("hidden")))
#endif
#ifndef QTR_EXT2_LIB  // likewise the second extension library's (include/quatro_place_batch.h)
#define QTR_EXT2_API __attribute__((visibility("hidden")))
#endif
#ifndef QTR_EXT3_LIB  // likewise the third extension library's (include/quatro_voxelmap_ct.h)
#define QTR_EXT3_API __attribute__((visibility("hidden")))
#endif
#include "solver.hip"
#include "exact.hip"
#include "stages.hip"
#include "frontend.hip"
#include "match.hip"
#include "keyframe.hip"
#include "place.hip"
#include "segment.hip"
#include "patchwork.hip"
#include "icp.hip"
#include "eval.hip"
#include "pgo.hip"
#include "capi.hip"
#include "voxelmap.hip"
#include "voxelmap_keep.hip"
#include "voxelmap_carve.hip"
#include "voxelmap_group.hip"
#include "voxelmap_batch.hip"
#include "voxelmap_eval.hip"
#include "deskew.hip"
#include "formats.hip"
#include "place_batch.hip"
#include "voxelmap_ct.hip"
