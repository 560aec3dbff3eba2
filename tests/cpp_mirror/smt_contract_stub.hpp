// What mirror_contract_main.cpp sees of smt_contract_stub.cpp besides include/smt.h.
#pragma once
#include <string>
#include <vector>

struct StubCall {
    std::string entry;
    std::vector<long long> args;   // the scalar arguments in the entry's order (sizes, counts, view, form, ...)
};

// every call of a stubbed entry since the last stub_log_clear(), plumbing (malloc, memcpy, sync) included
const std::vector<StubCall> &stub_log();
void stub_log_clear();
// the next call of `entry` returns rc and touches no memory
void stub_fail(const char *entry, int rc);
// the next call of `entry` raises the flag it keeps in device memory (ub_flag, err_dev); a flag is not a return value
void stub_flag(const char *entry);
// the byte every element of output number k of `entry` is filled with (1..200; class maps of the LR checks hold i % 3)
unsigned char stub_pattern(const char *entry, int k);
// handles created and not destroyed, device allocations not freed, streams not destroyed
int stub_live_handles();
int stub_live_allocs();
int stub_live_streams();
