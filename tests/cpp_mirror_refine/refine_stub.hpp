// What tests/cpp_mirror_refine/refine_mirror_main.cpp may ask of the stub besides the C ABI.
#pragma once
#include <string>
#include <vector>

// the byte every element of an output is filled with
enum : unsigned char { STUB_MAP = 0x5A, STUB_STATE = 0x3C, STUB_STATUS = 0x17 };

struct StubCall { int pairs, H, W, D, irv_ts, irv_iters, search; float irv_th; bool arms, cls, state, status; };

const std::vector<std::string> &stub_log();   // the entries called, in order
void stub_log_clear();
void stub_fail(const char *entry);            // the next call of `entry` returns SMT_ERR_HIP
int stub_live_allocs();
const StubCall &stub_last_refine();           // the arguments of the last voting / interpolation / refine entry
unsigned stub_last_arm_quirks();               // the quirk bits of the handle of the last smt_crossarm_arms
