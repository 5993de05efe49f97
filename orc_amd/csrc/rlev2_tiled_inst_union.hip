// rlev2_tiled_kernel instances (rlev2_tiled.cpp kInstances): the union
// instances, two passes and one.
#include "rlev2_tiled_kernel.hh"

namespace orcg {
ORCG_TILED_UNIT(union)
template void enqueue<kSer | kOptUnion | kOptTable, 8, 6, 2, 0>(Ctx*, const TiledLaunch&);
template void enqueue<kSer | kOptUnion, 8, 6, 2, 0>(Ctx*, const TiledLaunch&);
}  // namespace orcg
