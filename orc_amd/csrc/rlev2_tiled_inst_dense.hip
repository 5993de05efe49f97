// rlev2_tiled_kernel instances (rlev2_tiled.cpp kInstances): the two
// dense-capable instances.
#include "rlev2_tiled_kernel.hh"

namespace orcg {
ORCG_TILED_UNIT(dense)
template void enqueue<kSer, 8, 6, 2, 0>(Ctx*, const TiledLaunch&);
template void enqueue<kSer, 12, 5, 2, 0>(Ctx*, const TiledLaunch&);
}  // namespace orcg
