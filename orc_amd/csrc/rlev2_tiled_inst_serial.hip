// rlev2_tiled_kernel instances (rlev2_tiled.cpp kInstances): the serial-walk
// instances, that is the 33 KB register-filled family and the 21 KB one, and
// the dense drain of the two of them that queue.
#include "rlev2_tiled_kernel.hh"

namespace orcg {
ORCG_TILED_UNIT(serial)
template void enqueue<kWide | kOptFlat | kOptFlat16, 33, 1, 0, 0>(Ctx*, const TiledLaunch&);
template void enqueue<kWide, 33, 1, 0, 1>(Ctx*, const TiledLaunch&);
template void enqueue<kWide, 33, 1, 0, 0>(Ctx*, const TiledLaunch&);
template void enqueue<kWide | kOptFlat, 33, 1, 0, 0>(Ctx*, const TiledLaunch&);
template void enqueue<kSer, 21, 6, 0, 1>(Ctx*, const TiledLaunch&);
template void enqueue<kSer, 8, 6, 2, 2>(Ctx*, const TiledLaunch&);
}  // namespace orcg
