// shape_tables.cpp -- prints the launch-shape tables of llm-qat_amd/csrc/fq_shapes.h as the launch layer reads them (host program, no HIP):
//   reg <nvec> <threads per row> <vectors per thread>      by_reg_shape, nvec = 1 .. REG_MAX_VEC
//   group <nvec> <threads per row> <vectors per thread>    by_group_shape, the same range
//   count <n> <served 0/1>                                 by_count, n = 0 .. 9
// tests/test_shape_tables_cpu.py compiles it (g++ -std=c++17) and compares the tests' Python mirrors with what it prints.
#include <cstdio>

#include "fq_shapes.h"

int main() {
    for (long long nvec = 1; nvec <= fq::REG_MAX_VEC; ++nvec)
        fq::by_reg_shape(nvec, [&](auto tpr, auto vpt) { std::printf("reg %lld %d %d\n", nvec, decltype(tpr)::value, decltype(vpt)::value); });
    for (long long nvec = 1; nvec <= fq::REG_MAX_VEC; ++nvec)
        fq::by_group_shape(nvec, [&](auto tpr, auto vpt) { std::printf("group %lld %d %d\n", nvec, decltype(tpr)::value, decltype(vpt)::value); });
    for (int n = 0; n <= 9; ++n) {
        int served = 0;
        fq::by_count(n, [&](auto c) { served = decltype(c)::value == n; });
        std::printf("count %d %d\n", n, served);
    }
    return 0;
}
