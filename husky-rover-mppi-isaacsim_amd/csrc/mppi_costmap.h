// On-device obstacle costmap builder:
// Surface.create_obstacles_costmap, thesis_master/warp_implementation/MPPI_isaac.py:361-378.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mppi {

// Device scratch for one build of a size x size costmap (grown on demand by the caller).
struct CostmapScratch {
  uint8_t* occ = nullptr;    // [size*size] 1 = inside an inflated obstacle disc
  int32_t* first = nullptr;  // [segments*size] first occupied row of each column segment (-1: none)
  int32_t* last = nullptr;   // [segments*size] last occupied row of each column segment (-1: none)
  int32_t* g2 = nullptr;     // [size*size] squared vertical distance to the nearest obstacle (column pass)
  int32_t* d2 = nullptr;     // [size*size] squared Euclidean distance (row pass)
  int32_t* range = nullptr;  // [2] min / max of d2 (exact), then [2][COSTMAP_PARTIALS] chamfer min / max partials
  uint32_t* lines = nullptr; // [16*size*size] chamfer line scans: 8 knight planes, 8 axial/diagonal planes
  double* obs = nullptr;     // [n*3] (x_local, y_local, total_radius) per obstacle
  double* xs = nullptr;      // [size] np.linspace(-hw, hw, size)
  size_t cells_cap = 0, obs_cap = 0, xs_cap = 0;
};

constexpr int COSTMAP_PARTIALS = 1024;  // = CL_PART in mppi_costmap.hip
constexpr int COSTMAP_SEG = 32;         // rows per column segment of the column pass
constexpr int COSTMAP_MAX_SIZE = 8192;  // (2*size+1)^2 must fit int32 (the no-obstacle marker)

// distance metric of the build
constexpr int COSTMAP_CHAMFER5 = 0;  // cv2.distanceTransform(DIST_L2, 5), the reference (default)
constexpr int COSTMAP_EXACT = 1;     // exact Euclidean distance
constexpr int COSTMAP_CHAMFER5_RASTER = 2;  // the chamfer by the row-serial raster kernel (same result)

// The steep cells of a DEM as further occupied cells (the host side is
// mppi_hazard.h).  The passes borrow the scratch planes before the metric needs them: the int32
// count plane is sc.d2, the H0 occupancy the first size*size bytes of sc.lines.
struct CostmapHazard {
  const float* Z = nullptr;     // [rows*cols] heights, device, read in place
  int rows = 0, cols = 0;
  float res = 0;                // DEM resolution (the normal's vz = res^2)
  float cos_limit = 0;          // steep iff !(nz >= cos_limit)
  const int32_t* ci = nullptr;  // [cols] costmap column of a DEM column (-1: outside), device
  const int32_t* rj = nullptr;  // [rows] costmap row of a DEM row (-1: outside), device
  int32_t min_cells = 1;        // H0 = count >= min_cells
  int32_t T = 0;                // H1 = squared cell distance to H0 <= T
  int rows_per_group = 8;       // count kernel tiling (hazard_tiling)
  bool lds = true;
  uint8_t* mask = nullptr;      // [size*size] optional: bit 0 H0, bit 1 H1, bit 2 rock disc
  hipEvent_t ev_count[2] = {nullptr, nullptr};  // optional: recorded around the count kernel
};

// Enqueue the whole build on `st`: raster -> distance (chamfer: 16 independent line scans, or the
// two raster passes on one workgroup for a map without obstacle cells / COSTMAP_CHAMFER5_RASTER;
// exact: column pass, row pass) -> min/max -> min-max normalise -> (1 - d)^power, written to
// out[size*size] (device, float32, row-major).  sc.obs / sc.xs must already hold the n obstacle
// triples and the size grid coordinates.  With `hz`, between the raster and the distance: count the
// steep DEM cells per costmap cell -> H0 -> (T > 0: the exact column and row passes on H0) -> H1
// ORed into the occupancy; without it the launches are exactly those listed above.
hipError_t launch_costmap_build(const CostmapScratch& sc, int n_obs, int size, int power, float* out,
                                hipStream_t st, int metric, const CostmapHazard* hz = nullptr);

}  // namespace mppi
