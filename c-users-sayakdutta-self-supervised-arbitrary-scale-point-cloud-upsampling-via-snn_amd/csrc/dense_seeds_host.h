// The host flood's own fan distance and 6-decimal rounding, for csrc/dense_seeds_dev.hip (inside the library only, not part of
// the C ABI): the device flood hands a voxel to these when the host's result depends on its k-d traversal (an exact tie between
// the 10th and 11th nearest point) or when its x index lies outside the uploaded 6-decimal table.
#pragma once
#include <stdint.h>

namespace sapcu_seeds {

struct HostFan;                                                    // the n+1 points (the cloud + the all-zero point) and their k-d tree
HostFan* host_fan_create(const double* cloud_host, int64_t n);
double host_fan_distance(const HostFan* f, double cx, double cy, double cz);
void host_fan_destroy(HostFan* f);
double host_six_decimals(double x);

}  // namespace sapcu_seeds
