// What tests/cpp_mirror_fill_holes/fill_holes_mirror_main.cpp may ask of the stub besides the C ABI.
#pragma once
#include <string>
#include <vector>

// the byte every element of an output is filled with
enum : unsigned char { STUB_MAP = 0x5A, STUB_STATUS = 0x17 };

struct StubCall { int pairs, H, W; float invalid; bool status; std::vector<unsigned char> cls; };

const std::vector<std::string> &stub_log();   // the entries called, in order
void stub_log_clear();
void stub_fail(const char *entry);            // the next call of `entry` returns SMT_ERR_HIP
int stub_live_allocs();
const StubCall &stub_last_fill();             // the arguments of the last smt_fill_holes_batch, its class map copied
