// `name=value` arguments, one definition for the six tools: the error exit of the reference convention (message
// on stdout, exit(0)), the split of argv[i], the strict value parsers, and a key table -- one line per key: name, kind,
// destination, bounds -- with one loop over it.  Two families of kinds live side by side:
//   strict (bpmix, bpeval): a value that does not parse or is out of bounds ends the run with `TOOL: bad value for K: V`, or with
//     `K: V <tail>` where the key has a text of its own;
//   lenient (bptrain, bpforward, bpenhance, bpfeat): atoi / atof as the reference's Interface.cc reads them, so fea_dim=12abc is 12.
// Which keys a tool does not know is its own business: key_apply only says that it found none.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../../include/bp_c_api.h"

namespace bp {

[[noreturn]] inline void fail(const std::string &msg)
{
    printf("%s\n", msg.c_str());
    exit(0);
}

inline void check(int rc)
{
    if (rc != 0) fail(bp_last_error());
}

struct Arg { std::string k, v; };
inline Arg split_arg(const char *arg)
{
    const char *eq = strchr(arg, '=');
    if (!eq) fail(std::string("Arg: ") + arg + "  Format Error");
    return {std::string(arg, eq - arg), std::string(eq + 1)};
}

// ---- strict parsers: the whole value, nothing else
inline bool parse_int(const std::string &v, long lo, long hi, int *out)
{
    char *end = nullptr;
    const long n = strtol(v.c_str(), &end, 10);
    if (v.empty() || *end || n < lo || n > hi) return false;
    *out = (int)n;
    return true;
}
inline bool parse_double(const std::string &v, double *out)
{
    char *end = nullptr;
    const double d = strtod(v.c_str(), &end);
    if (v.empty() || *end || !std::isfinite(d)) return false;
    *out = d;
    return true;
}
inline bool parse_float(const std::string &v, float *out)
{
    double d = 0.0;
    if (!parse_double(v, &d)) return false;
    *out = (float)d;
    return true;
}
inline bool parse_u64(const std::string &v, unsigned long long *out)
{
    char *end = nullptr;
    const unsigned long long n = strtoull(v.c_str(), &end, 10);
    if (v.empty() || *end || v[0] == '-') return false;
    *out = n;
    return true;
}
// field i of a comma list at pos; false after the last one
inline bool next_field(const std::string &v, size_t *pos, std::string *field)
{
    if (*pos == std::string::npos) return false;
    const size_t c = v.find(',', *pos);
    *field = v.substr(*pos, c == std::string::npos ? c : c - *pos);
    *pos = c == std::string::npos ? c : c + 1;
    return true;
}
// exactly n finite numbers
inline bool parse_doubles(const std::string &v, int n, double *out)
{
    size_t pos = 0;
    std::string f;
    for (int i = 0; i < n; ++i)
        if (!next_field(v, &pos, &f) || !parse_double(f, &out[i])) return false;
    return pos == std::string::npos;
}
// 1..max ints in [lo, hi]
inline bool parse_ints(const std::string &v, long lo, long hi, int max, int *out, int *n)
{
    size_t pos = 0;
    std::string f;
    for (*n = 0; next_field(v, &pos, &f); ++*n)
        if (*n == max || !parse_int(f, lo, hi, &out[*n])) return false;
    return true;
}
inline bool parse_floats(const std::string &v, std::vector<float> *out)
{
    size_t pos = 0;
    std::string f;
    out->clear();
    for (float x = 0; next_field(v, &pos, &f); out->push_back(x))
        if (!parse_float(f, &x)) return false;
    return true;
}

// ---- the key table
enum Kind {
    K_STR,                                                       // std::string
    // strict
    K_INT,                                                       // int in [lo, hi]
    K_FLOAT,                                                     // finite float; in [lo, hi] where lo < hi
    K_U64,                                                       // unsigned long long, no sign
    K_CHOICE,                                                    // one of names ("a|b|c") -> int lo, lo + 1, ...
    K_SIZES,                                                     // 1..hi ints in [1, 2^20] -> int[], *count
    K_FLOATS,                                                    // comma list -> std::vector<float>
    // lenient (Interface.cc)
    K_ATOI, K_ATOF,                                              // int, float
    K_NONZERO,                                                   // int: atoi != 0
    K_IS, K_ISNT,                                                // int: v == names, v != names
    K_STRTOULL,                                                  // unsigned long long, whatever strtoull makes of it
    K_ATOI_SIZES                                                 // atoi per field, appended to int[] while *count < hi
};
struct Key {
    const char *name;
    Kind kind;
    void *dst;
    double lo, hi;
    const char *names;                                           // K_CHOICE, K_IS, K_ISNT
    const char *tail;                                            // the key's own text: `K: V <tail>` in place of `bad value`
    int *count;                                                  // K_SIZES, K_ATOI_SIZES
};

inline bool key_value(const Key &K, const std::string &v)
{
    switch (K.kind) {
    case K_STR: *(std::string *)K.dst = v; return true;
    case K_INT: return parse_int(v, (long)K.lo, (long)K.hi, (int *)K.dst);
    case K_FLOAT: return parse_float(v, (float *)K.dst) && (!(K.lo < K.hi) || (*(float *)K.dst >= (float)K.lo && *(float *)K.dst <= (float)K.hi));
    case K_U64: return parse_u64(v, (unsigned long long *)K.dst);
    case K_CHOICE: {
        size_t pos = 0;
        const std::string names(K.names);
        for (int i = 0; pos <= names.size(); ++i) {
            const size_t bar = std::min(names.find('|', pos), names.size());
            if (names.compare(pos, bar - pos, v) == 0) { *(int *)K.dst = (int)K.lo + i; return true; }
            pos = bar + 1;
        }
        return false;
    }
    case K_SIZES: return parse_ints(v, 1, 1 << 20, (int)K.hi, (int *)K.dst, K.count);
    case K_FLOATS: return parse_floats(v, (std::vector<float> *)K.dst);
    case K_ATOI: *(int *)K.dst = atoi(v.c_str()); return true;
    case K_ATOF: *(float *)K.dst = (float)atof(v.c_str()); return true;
    case K_NONZERO: *(int *)K.dst = atoi(v.c_str()) != 0; return true;
    case K_IS: *(int *)K.dst = v == K.names; return true;
    case K_ISNT: *(int *)K.dst = v != K.names; return true;
    case K_STRTOULL: *(unsigned long long *)K.dst = strtoull(v.c_str(), 0, 10); return true;
    case K_ATOI_SIZES: {
        size_t pos = 0;
        std::string f;
        while (*K.count < (int)K.hi && next_field(v, &pos, &f)) ((int *)K.dst)[(*K.count)++] = atoi(f.c_str());
        return true;
    }
    }
    return false;
}

[[noreturn]] inline void bad_value(const char *tool, const std::string &k, const std::string &v)
{
    fail(std::string(tool) + ": bad value for " + k + ": " + v);
}

// false: k is not in the table.  A value the key does not take ends the run.
template <size_t N>
inline bool key_apply(const Key (&keys)[N], const char *tool, const Arg &a)
{
    for (const Key &K : keys) {
        if (a.k != K.name) continue;
        if (!key_value(K, a.v)) {
            if (K.tail) fail(a.k + ": " + a.v + " " + K.tail);
            bad_value(tool, a.k, a.v);
        }
        return true;
    }
    return false;
}

// rate=R as the four WAV tools take it: one range, and in the lenient tools one text
const long RATE_MAX = 1L << 30;
const char *const RATE_TAIL = "is not a sample rate >= 1";

// lm_noise=vad|spp as bpenhance (tail: its own text) and bpeval (tail null: `bad value`) take it: the noise
// update of the log-MMSE baseline, BP_NOISE_VAD or BP_NOISE_SPP
inline bool lm_noise_key(const Arg &a, const char *tool, const char *tail, int *mode)
{
    const Key keys[] = {{"lm_noise", K_CHOICE, mode, BP_NOISE_VAD, 0, "vad|spp", tail}};
    return key_apply(keys, tool, a);
}

// nat=static|dynamic as bpenhance (tail: its own text), bpmix and bpeval (tail null: `bad value`) take it: the
// noise-aware block of the net's input, BP_NAT_STATIC or BP_NAT_DYNAMIC; net_setup.h's set_nat hands it to the handle
inline bool nat_key(const Arg &a, const char *tool, const char *tail, int *mode)
{
    const Key keys[] = {{"nat", K_CHOICE, mode, BP_NAT_STATIC, 0, "static|dynamic", tail}};
    return key_apply(keys, tool, a);
}

// post_gv=FILE post_mask_col= post_mask_lo= post_mask_hi= post_mask_weight= as bpenhance (tails: its own texts) and
// bpeval (tails off: `bad value`) take them: post-processing of the net's LPS estimate, GV factors from the file that
// `bpeval gv_out=` writes and the mask gate; net_setup.h's set_post hands them to the handle
struct PostKeys {
    std::string gv;                                              // post_gv: centre then scale, in norm-file format
    int mask_col = -1;
    float lo = 0.5f, hi = 0.5f, weight = 1.0f;
    bool gate_given = false;                                     // post_mask_lo, _hi or _weight was given
    bool on() const { return !gv.empty() || mask_col >= 0; }
};
inline bool post_key(const Arg &a, const char *tool, bool tails, PostKeys *p)
{
    const Key keys[] = {
        {"post_gv", K_STR, &p->gv},
        {"post_mask_col", K_INT, &p->mask_col, 0, 1 << 20, nullptr, tails ? "is not a column >= 0" : nullptr},
        {"post_mask_lo", K_FLOAT, &p->lo, 0, 0, nullptr, tails ? "is not a finite number" : nullptr},
        {"post_mask_hi", K_FLOAT, &p->hi, 0, 0, nullptr, tails ? "is not a finite number" : nullptr},
        {"post_mask_weight", K_FLOAT, &p->weight, 0, 1, nullptr, tails ? "is not a number in [0, 1]" : nullptr},
    };
    if (!key_apply(keys, tool, a)) return false;
    if (a.k != "post_gv" && a.k != "post_mask_col") p->gate_given = true;
    return true;
}
// what the keys must satisfy together, before the device is used
inline void check_post_keys(const char *tool, const PostKeys &p, int wave_target)
{
    if (p.gate_given && p.mask_col < 0) fail(std::string(tool) + ": post_mask_lo, post_mask_hi and post_mask_weight need post_mask_col");
    if (p.lo > p.hi) fail(std::string(tool) + ": post_mask_lo must not exceed post_mask_hi");
    if (p.on() && wave_target != BP_WAVE_LPS) fail(std::string(tool) + ": post_gv and post_mask_col need wave_target=lps");
}

// output_act / output_linear_dims / output_loss as bptrain, bpforward and bpenhance take them: strict, with their own texts (a
// typo must not silently run a different model)
inline bool output_key(const Arg &a, int *act, int *dims, int *loss)
{
    const Key keys[] = {
        {"output_act", K_CHOICE, act, 0, 0, "linear|sigmoid", "is not linear or sigmoid"},
        {"output_linear_dims", K_INT, dims, 0, 1000000, nullptr, "is not a column count"},
        {"output_loss", K_CHOICE, loss, 0, 0, "xent|mse", "is not xent or mse"},
    };
    return key_apply(keys, "", a);
}

}  // namespace bp
