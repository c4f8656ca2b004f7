// call_parts.h - the small host pieces every tiled back end writes the same way: the rounding of a staging offset, the entry of a
// flattened tile list, and the limit of a frame's side.  No HIP here: backend.h brings them to the .hip files, and the HIP-free headers
// (ingest_host.h, facemask_host.h) and the stand-alone checks under tools/ include this file alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rtd {
namespace backend {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// one workgroup's work: a tile of the thing `owner` indexes (a frame of the ingest and the overlays, a face of the face masks)
struct TileRef {
  int32_t owner, tile;       // tile = ty * tiles_x + tx of the owner's descriptor
};

// the sides of every frame, crop source and output: 1..65535 (a tile index and a byte offset inside a row then fit 32 bits)
constexpr int64_t MAX_SIDE = 65535;
inline bool sides_ok(int64_t a, int64_t b) { return a >= 1 && b >= 1 && a <= MAX_SIDE && b <= MAX_SIDE; }

}  // namespace backend
}  // namespace rtd
