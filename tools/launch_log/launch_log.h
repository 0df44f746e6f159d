// Host-side launch log: what would a translation unit of libamdnuwa launch, and with which arguments?
//
//     hipcc ... -include tools/launch_log/launch_log.h FILE.hip        (tools/launch_log/run.py does this)
//
// turns hipFuncSetAttribute, hipLaunchKernelGGL, hipGetLastError, hipMemsetAsync and hipMemcpyAsync of that file into a logger: nothing reaches a device, so
// the entry points can be walked with fake operand pointers on a machine without a GPU.  One line per call:
//
//     attr   <kernel> <attribute> <value>
//     launch <kernel> grid x y z block x y z lds <bytes> args <64-bit FNV-1a of the argument bytes>
//     memset <value> <bytes>
//     memcpy <bytes> <kind>
//
// <kernel> is the offset of the host-side kernel handle inside the scratch library ("+0x..."); run.py turns it into the symbol through the
// library's symbol table.  Every argument is converted to the kernel's own parameter type before it is hashed, so the hash does not depend
// on how the call site spells a value.  The pointer VALUES are hashed: the driver passes the same fake addresses to both trees.
// launch_log_take() hands the lines collected since the last call to the driver.  Not part of the library, the build or the test suite.
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <type_traits>

namespace launch_log {

inline std::string& lines() { static std::string s; return s; }

inline std::string kernel_id(const void* k) {
    Dl_info info;
    char buf[64];
    if (dladdr(k, &info) && info.dli_fbase) snprintf(buf, sizeof buf, "+0x%zx", (size_t)((const char*)k - (const char*)info.dli_fbase));
    else snprintf(buf, sizeof buf, "?%p", k);
    return buf;
}

inline void fnv(uint64_t& h, const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; }
}
template <class P, class A> void hash_arg(uint64_t& h, const A& a) {
    static_assert(std::is_trivially_copyable<P>::value, "kernel parameters are plain data");
    if constexpr (std::is_same<P, std::decay_t<A>>::value) fnv(h, &a, sizeof(P));       // the caller's bytes, padding included
    else { const P v = a; fnv(h, &v, sizeof(P)); }
}

template <class... P, class... A>
void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t, const A&... args) {
    static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
    uint64_t h = 14695981039346656037ull;
    (hash_arg<P>(h, args), ...);
    char buf[256];
    snprintf(buf, sizeof buf, "launch %s grid %u %u %u block %u %u %u lds %zu args %016llx\n", kernel_id((const void*)kernel).c_str(), grid.x, grid.y,
             grid.z, block.x, block.y, block.z, lds, (unsigned long long)h);
    lines() += buf;
}
inline hipError_t attr(const void* kernel, hipFuncAttribute a, int value) {
    char buf[128];
    snprintf(buf, sizeof buf, "attr %s %d %d\n", kernel_id(kernel).c_str(), (int)a, value);
    lines() += buf;
    return hipSuccess;
}
inline hipError_t memset_async(void*, int value, size_t bytes, hipStream_t) {
    char buf[96];
    snprintf(buf, sizeof buf, "memset %d %zu\n", value, bytes);
    lines() += buf;
    return hipSuccess;
}
inline hipError_t memcpy_async(void*, const void*, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    char buf[96];
    snprintf(buf, sizeof buf, "memcpy %zu %d\n", bytes, (int)kind);
    lines() += buf;
    return hipSuccess;
}

}  // namespace launch_log

// copies the pending lines (NUL-terminated, cut at n - 1 bytes) into buf, forgets them, returns their full length
extern "C" __attribute__((visibility("default"), weak)) size_t launch_log_take(char* buf, size_t n) {
    std::string& s = launch_log::lines();
    const size_t len = s.size();
    if (buf && n) { const size_t c = len < n - 1 ? len : n - 1; memcpy(buf, s.data(), c); buf[c] = 0; }
    s.clear();
    return len;
}

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(...) ::launch_log::launch(__VA_ARGS__)
#define hipFuncSetAttribute(...) ::launch_log::attr(__VA_ARGS__)
#define hipGetLastError() hipSuccess
#define hipMemsetAsync(...) ::launch_log::memset_async(__VA_ARGS__)
#define hipMemcpyAsync(...) ::launch_log::memcpy_async(__VA_ARGS__)
