// What tests/cpp_mirror_scan_views/scan_views_main.cpp may ask of the stub besides the C ABI.
#pragma once
#include <string>
#include <vector>

// the byte every element of an output is filled with
enum : unsigned char { STUB_VOUT_L = 0x11, STUB_VOUT_R = 0x22, STUB_DISP_L = 0x33, STUB_DISP_R = 0x44, STUB_DISP_R_LEFT = 0x55, STUB_CLS = 0x02 };

const std::vector<std::string> &stub_log();   // the entries called, in order
void stub_log_clear();
void stub_fail(const char *entry);            // the next call of `entry` returns SMT_ERR_HIP
int stub_live_allocs();
int stub_live_handles();
