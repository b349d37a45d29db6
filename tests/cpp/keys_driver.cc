// The value parsers and key kinds of csrc/host/keys.h on their own (tests/test_cli_host.py builds this with
// -fsanitize=address,undefined and runs it on the CPU): a table of strings per parser with what each must make of it.  The
// expectations are those of strtol / strtod / strtoull on an LP64 machine, written down here, not taken from a run.
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <string>
#include <vector>

#include "host/keys.h"

static int g_bad = 0;
static void expect(bool ok, const char *what, const std::string &v)
{
    if (ok) return;
    ++g_bad;
    printf("FAIL %s on \"%s\"%s\n", what, v.substr(0, 40).c_str(), v.size() > 40 ? "..." : "");
}

int main()
{
    using namespace bp;
    const std::string digits(65536, '7');
    const unsigned long long U64MAX = std::numeric_limits<unsigned long long>::max();
    // ---- the eight strings every scalar parser sees: ok and value per parser
    struct Row { std::string v; bool i_ok; int i; bool f_ok; float f; bool u_ok; unsigned long long u; };
    const Row rows[] = {
        {"", false, 0, false, 0, false, 0},
        {"-0", true, 0, true, -0.0f, false, 0},                                      // (u64 refuses the sign)
        {"+5", true, 5, true, 5.0f, true, 5},
        {"1e400", false, 0, false, 0, false, 0},                                     // int/u64: stops at e; float: inf
        {"nan", false, 0, false, 0, false, 0},
        {"2147483648", false, 0, true, 2147483648.0f, true, 2147483648ull},          // int: above hi
        {"18446744073709551616", false, 0, true, 18446744073709551616.0f, true, U64MAX},   // strtoull saturates: taken, as it always was
        {digits, false, 0, false, 0, true, U64MAX},                                  // float: inf
    };
    for (const Row &r : rows) {
        int i = -7;
        float f = -7;
        unsigned long long u = 7;
        expect(parse_int(r.v, 0, 2147483647L, &i) == r.i_ok && i == (r.i_ok ? r.i : -7), "parse_int", r.v);
        expect(parse_float(r.v, &f) == r.f_ok && f == (r.f_ok ? r.f : -7.0f), "parse_float", r.v);
        expect(parse_u64(r.v, &u) == r.u_ok && u == (r.u_ok ? r.u : 7), "parse_u64", r.v);
    }
    {
        float f = 1;
        expect(parse_float("-0", &f) && std::signbit(f), "parse_float sign of", "-0");
        int i = 0;
        expect(parse_int("-3", -3, 3, &i) && i == -3, "parse_int", "-3");
        expect(!parse_int("-4", -3, 3, &i) && !parse_int("4", -3, 3, &i) && !parse_int("3 ", -3, 3, &i) && !parse_int("0x1", -3, 3, &i), "parse_int bounds/tail", "-4 4 '3 ' 0x1");
        expect(parse_int(" 3", -3, 3, &i) && i == 3, "parse_int (strtol skips leading blanks)", " 3");
    }
    // ---- lists
    {
        double d[3] = {0, 0, 0};
        expect(parse_doubles("1,2.5", 2, d) && d[0] == 1.0 && d[1] == 2.5, "parse_doubles", "1,2.5");
        for (const char *v : {"", "1", "1,2,3", "1,,2", "1,2,", ",1", "1,x", "1,inf", digits.c_str()}) expect(!parse_doubles(v, 2, d), "parse_doubles(2)", v);
        expect(parse_doubles("0.5", 1, d) && !parse_doubles("0.5,", 1, d), "parse_doubles(1)", "0.5");
        int s[4] = {0, 0, 0, -1}, n = 0;
        expect(parse_ints("1,20,300", 1, 1 << 20, 3, s, &n) && n == 3 && s[0] == 1 && s[1] == 20 && s[2] == 300 && s[3] == -1, "parse_ints", "1,20,300");
        for (const char *v : {"", "1,2,3,4", "1,,2", "1,", "0", "1048577", "1,x", digits.c_str()}) expect(!parse_ints(v, 1, 1 << 20, 3, s, &n) && s[3] == -1, "parse_ints(3)", v);
        std::vector<float> f;
        expect(parse_floats("-5,0,2.5", &f) && f.size() == 3 && f[0] == -5.0f && f[2] == 2.5f, "parse_floats", "-5,0,2.5");
        for (const char *v : {"", "1,", ",", "1,nan", "1e400", digits.c_str()}) expect(!parse_floats(v, &f), "parse_floats", v);
        std::string many;
        for (int k = 0; k < 20000; ++k) many += "1,";
        expect(parse_floats(many + "2", &f) && f.size() == 20001, "parse_floats", "20001 fields");
    }
    // ---- kinds
    {
        int c = -1;
        const Key choice = {"k", K_CHOICE, &c, 4, 0, "a|bc|d"};
        expect(key_value(choice, "a") && c == 4, "K_CHOICE", "a");
        expect(key_value(choice, "bc") && c == 5, "K_CHOICE", "bc");
        expect(key_value(choice, "d") && c == 6, "K_CHOICE", "d");
        for (const char *v : {"", "b", "c", "a|bc", "|", "bcd", "A", digits.c_str()}) expect(!key_value(choice, v) && c == 6, "K_CHOICE", v);
        float f = 0;
        const Key bounded = {"k", K_FLOAT, &f, 0, 1e6}, open = {"k", K_FLOAT, &f};
        expect(key_value(bounded, "0") && key_value(bounded, "1e6") && !key_value(bounded, "-1e-3") && !key_value(bounded, "1000001"), "K_FLOAT bounds", "0 1e6 -1e-3 1000001");
        expect(key_value(open, "-1e30") && f == -1e30f && !key_value(open, "inf"), "K_FLOAT", "-1e30 inf");
        int i = 0;
        const Key ai = {"k", K_ATOI, &i}, nz = {"k", K_NONZERO, &i}, is = {"k", K_IS, &i, 0, 0, "sigmoid"}, isnt = {"k", K_ISNT, &i, 0, 0, "host"};
        expect(key_value(ai, "129abc") && i == 129, "K_ATOI", "129abc");
        expect(key_value(ai, "x") && i == 0, "K_ATOI", "x");
        expect(key_value(ai, "") && i == 0, "K_ATOI", "");
        expect(key_value(nz, "2") && i == 1 && key_value(nz, "no") && i == 0, "K_NONZERO", "2 no");
        expect(key_value(is, "sigmoid") && i == 1 && key_value(is, "Sigmoid") && i == 0, "K_IS", "sigmoid Sigmoid");
        expect(key_value(isnt, "host") && i == 0 && key_value(isnt, "") && i == 1, "K_ISNT", "host ''");
        float af = 0;
        const Key at = {"k", K_ATOF, &af};
        expect(key_value(at, "0.5x") && af == 0.5f && key_value(at, "x") && af == 0.0f, "K_ATOF", "0.5x x");
        unsigned long long u = 0;
        const Key su = {"k", K_STRTOULL, &u};
        expect(key_value(su, "12abc") && u == 12 && key_value(su, digits) && u == U64MAX, "K_STRTOULL", "12abc digits");
        int ls[10], n = 0;
        for (int &x : ls) x = -1;
        const Key sizes = {"k", K_ATOI_SIZES, ls, 0, 10, nullptr, nullptr, &n};
        expect(key_value(sizes, "3,,4,") && n == 4 && ls[0] == 3 && ls[1] == 0 && ls[2] == 4 && ls[3] == 0 && ls[4] == -1, "K_ATOI_SIZES", "3,,4,");
        expect(key_value(sizes, "1,2,3,4,5,6,7,8,9") && n == 10 && ls[4] == 1 && ls[9] == 6, "K_ATOI_SIZES appends up to hi", "1..9");
        expect(key_value(sizes, "5") && n == 10 && ls[9] == 6, "K_ATOI_SIZES when full", "5");
        int ss[9], sn = 0;
        const Key strict = {"k", K_SIZES, ss, 0, 9, nullptr, nullptr, &sn};
        expect(key_value(strict, "1,2,3,4,5,6,7,8,9") && sn == 9 && !key_value(strict, "1,2,3,4,5,6,7,8,9,10") && !key_value(strict, "99,64,") && !key_value(strict, "99,,33"), "K_SIZES", "9 / 10 / trailing / empty");
        std::string s;
        const Key str = {"k", K_STR, &s};
        expect(key_value(str, digits) && s == digits, "K_STR", digits);
    }
    {
        const Arg a = split_arg("a=b=c"), e = split_arg("=");
        expect(a.k == "a" && a.v == "b=c" && e.k.empty() && e.v.empty(), "split_arg", "a=b=c =");
    }
    if (!g_bad) printf("keys: every parser and kind agrees with its table\n");
    return g_bad ? 1 : 0;
}
