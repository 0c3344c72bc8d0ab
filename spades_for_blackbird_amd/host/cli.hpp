// cli.hpp -- the option table of the host tools: every tool lists its options once,
//   Options o;
//   o.num("-k", "--kmer", &K).str("-d", "--dataset", &dataset).flag("-h", "--help", &help).positional(&input);
//   const bool bad = !o.parse(argc, argv);
// and keeps its own usage text and its own condition for printing it.  An option has a short and a long name; either
// may be "".  parse() goes on after an error (it only decides usage versus run), a repeated option keeps its last value.
// Standard library only: tests/cli_check.cpp compiles this file alone.
#pragma once

#include <cstdlib>
#include <functional>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

namespace bbkhost {

// Decimal digits only (no sign, no blank), a value that fits T and lies in [lo, hi]; *out is written on success only.
template <class T>
inline bool parse_num(const char *s, T *out, T lo = 0, T hi = std::numeric_limits<T>::max()) {
    static_assert(std::is_unsigned<T>::value, "the tools' numeric options are unsigned");
    if (!s || !*s) return false;
    unsigned long long v = 0;
    for (; *s; ++s) {
        if (*s < '0' || *s > '9') return false;
        const unsigned d = (unsigned)(*s - '0');
        if (v > (std::numeric_limits<unsigned long long>::max() - d) / 10) return false;
        v = v * 10 + d;
    }
    if (v > std::numeric_limits<T>::max() || (T)v < lo || (T)v > hi) return false;
    *out = (T)v;
    return true;
}

class Options {
  public:
    // <name> <value>: an unsigned integer in [lo, hi]
    template <class T>
    Options &num(const char *s, const char *l, T *dst, T lo = 0, T hi = std::numeric_limits<T>::max()) {
        return add(s, l, [dst, lo, hi](const char *v) { return parse_num(v, dst, lo, hi); });
    }
    // <name> <value>: what strtod reads, all of the word
    Options &real(const char *s, const char *l, double *dst) {
        return add(s, l, [dst](const char *v) {
            char *end = nullptr;
            const double d = strtod(v, &end);
            if (end == v || *end) return false;
            *dst = d;
            return true;
        });
    }
    Options &str(const char *s, const char *l, std::string *dst) {
        return add(s, l, [dst](const char *v) { return *dst = v, true; });
    }
    // <name> <value>, accepted and dropped (the scratch directory of the reference's tools)
    Options &ignored(const char *s, const char *l) {
        return add(s, l, [](const char *) { return true; });
    }
    // <name> alone; the callback runs every time the flag is given
    Options &flag(const char *s, const char *l, std::function<void()> on) {
        opts_.push_back({s, l, false, [on](const char *) { return on(), true; }, false});
        return *this;
    }
    Options &flag(const char *s, const char *l, bool *dst) {
        return flag(s, l, [dst] { *dst = true; });
    }
    // Without this a bare word is an error; with it every word that does not start with '-', and "-" itself, is kept.
    Options &positional(std::vector<std::string> *dst) {
        pos_ = dst;
        return *this;
    }

    // false = usage error: an unknown option, a bare word nobody collects, a value that is missing or does not parse
    bool parse(int argc, char **argv) {
        bool ok = true;
        for (int i = 1; i < argc; ++i) {
            const std::string a = argv[i];
            const int at = find(a);
            Opt *o = at < 0 ? nullptr : &opts_[(size_t)at];
            if (o && !o->takes_value) o->seen = o->set(nullptr);
            else if (o) {
                if (i + 1 < argc && o->set(argv[++i])) o->seen = true;
                else ok = false;
            } else if (pos_ && (a.size() < 2 || a[0] != '-')) pos_->push_back(a);
            else ok = false;
        }
        return ok;
    }
    // whether the option was given (with a value that parsed), by either of its names
    bool seen(const std::string &name) const {
        const int i = find(name);
        return i >= 0 && opts_[(size_t)i].seen;
    }

  private:
    struct Opt {
        std::string s, l;
        bool takes_value;
        std::function<bool(const char *)> set;
        bool seen;
    };
    Options &add(const char *s, const char *l, std::function<bool(const char *)> set) {
        opts_.push_back({s, l, true, std::move(set), false});
        return *this;
    }
    int find(const std::string &name) const {
        for (size_t i = 0; i < opts_.size() && !name.empty(); ++i)
            if (name == opts_[i].s || name == opts_[i].l) return (int)i;
        return -1;
    }
    std::vector<Opt> opts_;
    std::vector<std::string> *pos_ = nullptr;
};

}  // namespace bbkhost
