// What tests/cpp_mirror_bilateral/bilateral_mirror_main.cpp may ask of the stub besides the C ABI.
#pragma once
#include <string>
#include <vector>

// the byte every element of an output is filled with
enum : unsigned char { STUB_DST = 0x5A, STUB_ACC = 0x3C };

struct StubCall { int images, H, W, channels, wsize_h, wsize_w, norm; bool acc; };

const std::vector<std::string> &stub_log();   // the entries called, in order
void stub_log_clear();
void stub_fail(const char *entry);            // the next call of `entry` returns SMT_ERR_HIP
int stub_live_allocs();
const StubCall &stub_last_filter();           // the arguments of the last smt_bilateral_filter_batch
