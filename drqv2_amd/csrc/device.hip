// The CU count every planner of the library sees: one per-device cache and one per-device override for the whole
// library (common.h declares drq_num_cus(); include/drqv2_hip.h holds the contract of the two entries).
#include "common.h"

namespace {
int g_hw_cus[kMaxDevices] = {};         // 0 = not asked yet
int g_override_cus[kMaxDevices] = {};   // 0 = none

int hardware_cus(int dev) {
  if (g_hw_cus[dev] == 0) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return 256;
    g_hw_cus[dev] = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
  }
  return g_hw_cus[dev];
}
}  // namespace

int drq_num_cus() {
  const int dev = drq_device();
  const int n = g_override_cus[dev];
  return n > 0 ? n : hardware_cus(dev);
}

DRQ_API int drq_num_cus_in_effect(void) { return drq_num_cus(); }

DRQ_API int drq_set_num_cus(int n) {
  const int dev = drq_device();
  if (n < 0 || n > hardware_cus(dev)) return DRQ_EARG;
  g_override_cus[dev] = n;
  return DRQ_OK;
}
