// instance_host.h - the instance frame's host helpers that need no handle (instance.hip defines them): what yh_engine's instance
// calls (instance.hip, instance_batch.hip, engine_ops.hip) and yh_tfl's (tfl_instance.hip, tflite_exec.hip) share. Not part of the C ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace yh __attribute__((visibility("hidden"))) {

const char* instance_check(int width, int height, const uint8_t* class_map, int ncls, float min_score);   // nullptr: fine
bool instance_grow_bytes(void** p, size_t* cap, size_t bytes);   // a device buffer that only grows (the old one is freed); false: hipMalloc failed, *p is nullptr
void instance_class_map(const uint8_t* class_map, int ncls, std::vector<uint8_t>& out);   // the call's class map, NULL resolved
void instance_table(const uint32_t* meta, std::vector<int32_t>& table);   // meta [2][128] as read back -> rows (rank, class, id, pixels)

}  // namespace yh
