// mesh_accel.h -- what the builder of the acceleration structure (mesh_accel_build.hip) and the query on it (mesh_accel_query.hip) share:
// the cluster size and the limits of the tables of VanerfMeshAccel (include/vanerf_hip.h).
#pragma once

namespace vanerf {

constexpr int CL = 4; // triangles (and vertices) per cluster.  Measured on the benchmark view: 16 -> 6.35 ms, 8 -> 4.80, 4 -> 4.37
                      // (box tests are cheap since they are done per wave first; small clusters mean fewer per-triangle tests)
constexpr int MA_MAX_CLUSTERS = 4096;  // triangle clusters: the query keeps their boxes in LDS and 16-bit ids in its candidate lists
constexpr int MA_MAX_VCLUSTERS = 1024; // vertex clusters: the query keeps the sorted vertices and their boxes in LDS

} // namespace vanerf
