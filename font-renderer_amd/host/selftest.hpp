// selftest.hpp — what the CPU self-tests of the host-only units share (host/*_selftest.cpp; each is one translation unit
// that links its unit's object and nothing else of the library): the fr::set_error the unit reports through, which here
// keeps the message for the line a refused case prints, and the helpers of the line formats and the property checks.
// The cases, the line formats and the properties are each program's own.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

namespace selftest {
inline char g_msg[512];
inline int g_failed = 0;
inline const char *last_error() { return g_msg; }          // of the calls since clear_error()
inline void clear_error() { g_msg[0] = 0; }
inline int exit_status() { return g_failed; }              // 1 once a require() has failed
}  // namespace selftest

namespace fr {
int set_error(int code, const char *f, ...)                // not inline: the unit's object calls it
{
    va_list ap;
    va_start(ap, f);
    vsnprintf(selftest::g_msg, sizeof selftest::g_msg, f, ap);
    va_end(ap);
    return code;
}
}  // namespace fr

namespace selftest {

// "a;b;c", or "-" for none
inline std::string join(const std::vector<std::string> &v)
{
    std::string s;
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ";" : "") + v[i];
    return s.empty() ? "-" : s;
}

inline std::string fmt(const char *f, ...)
{
    char b[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof b, f, ap);
    va_end(ap);
    return b;
}

// a property the kernels rely on: a failure names the case and the property on stderr and sets the exit status
inline void require(bool ok, const std::string &name, const char *what)
{
    if (ok) return;
    fprintf(stderr, "%s: %s\n", name.c_str(), what);
    g_failed = 1;
}

}  // namespace selftest
