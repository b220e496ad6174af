// host_check_util.hpp -- what the host harnesses of tests/ share: buffers with
// no slack, outputs between guard bytes, and the case reader (one case per line
// of stdin as key=value tokens; lists comma separated, bytes as hex).  Test
// code: the library never includes it.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace hostcheck {

constexpr uint8_t GUARD = 0xA5;
constexpr size_t FENCE = 64;  // guard bytes on either side of an output (a multiple of 16)

// n elements of T whose last byte is the last byte of a heap allocation, the
// first at `mis` bytes past a 16-byte aligned address (mis = 0: the allocation
// is exactly the n elements; else `mis` unused bytes lie before them)
template <class T>
struct Exact {
    uint8_t *raw = nullptr;
    T *p = nullptr;
    size_t n = 0;
    explicit Exact(size_t n_, uint32_t mis = 0) : n(n_) {
        void *q = nullptr;
        if (posix_memalign(&q, 16, mis + n * sizeof(T))) abort();
        raw = (uint8_t *)q;
        p = (T *)(raw + mis);
    }
    Exact(const std::vector<T> &v, uint32_t mis = 0) : Exact(v.size(), mis) {
        if (n) memcpy((void *)p, v.data(), n * sizeof(T));
    }
    Exact(const Exact &) = delete;
    ~Exact() { free(raw); }
    T &operator[](size_t i) { return p[i]; }
};

// n elements of T at `mis` bytes (rounded down to T's alignment) past a 16-byte aligned address, between guard bytes
template <class T>
struct Guarded {
    uint8_t *base = nullptr;
    size_t n, lead, bytes;
    Guarded(size_t n_, uint32_t mis = 0) : n(n_), lead(FENCE + (mis & ~(uint32_t)(alignof(T) - 1))) {
        bytes = lead + n_ * sizeof(T) + FENCE;
        void *q = nullptr;
        if (posix_memalign(&q, 16, bytes)) abort();
        base = (uint8_t *)q;
        memset(base, GUARD, bytes);
    }
    Guarded(const Guarded &) = delete;
    ~Guarded() { free(base); }
    T *view() { return (T *)(base + lead); }
    void fill(const std::vector<T> &v) {
        if (v.size()) memcpy(view(), v.data(), v.size() * sizeof(T));
    }
    bool intact() const {
        for (size_t i = 0; i < lead; ++i)
            if (base[i] != GUARD) return false;
        for (size_t i = lead + n * sizeof(T); i < bytes; ++i)
            if (base[i] != GUARD) return false;
        return true;
    }
};

struct Case {
    std::map<std::string, std::string> kv;
    bool has(const char *k) const { return kv.count(k) != 0; }
    uint64_t num(const char *k, uint64_t dflt) const {
        auto it = kv.find(k);
        return it == kv.end() ? dflt : strtoull(it->second.c_str(), nullptr, 10);
    }
    std::string str(const char *k) const {
        auto it = kv.find(k);
        return it == kv.end() ? std::string() : it->second;
    }
    template <class T>
    std::vector<T> list(const char *k) const {  // ("-1" reads as all ones)
        std::vector<T> out;
        auto it = kv.find(k);
        if (it == kv.end() || it->second.empty()) return out;
        const char *s = it->second.c_str();
        for (;;) {
            char *end;
            out.push_back((T)strtoull(s, &end, 10));
            if (*end != ',') break;
            s = end + 1;
        }
        return out;
    }
    std::vector<uint8_t> hex(const char *k) const {
        std::vector<uint8_t> out;
        auto it = kv.find(k);
        if (it == kv.end()) return out;
        const std::string &h = it->second;
        auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
        out.reserve(h.size() / 2);
        for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)(nib(h[i]) << 4 | nib(h[i + 1])));
        return out;
    }
};

inline void put_hex(const char *name, const uint8_t *p, size_t n, const char *end = ",") {
    static const char D[] = "0123456789abcdef";
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; ++i) s[2 * i] = D[p[i] >> 4], s[2 * i + 1] = D[p[i] & 15];
    printf("\"%s\":\"%s\"%s", name, s.c_str(), end);
}

template <class T>
void put_list(const char *name, const T *p, size_t n, const char *end = ",") {
    printf("\"%s\":[", name);
    for (size_t i = 0; i < n; ++i) printf("%s%llu", i ? "," : "", (unsigned long long)p[i]);
    printf("]%s", end);
}

// every line of stdin as a Case through `run`; its first non-zero result ends the program with it
template <class Run>
int run_lines(Run run) {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string tok;
        Case c;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 2;
            c.kv[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
        const int rc = run(c);
        if (rc) return rc;
        fflush(stdout);
    }
    return 0;
}

}  // namespace hostcheck
