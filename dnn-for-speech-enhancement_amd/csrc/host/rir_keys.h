// rir_rooms=N and the keys that go with it, one definition for bpmix and bpeval: simulated room impulse
// responses in place of rir_list.  The rooms are drawn by bp_rir_rooms from the tool's seed and checked on the host (the image
// count of bp_rir_image included), so every error is reported before the device is used; rir_generate is the one device call.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../../include/bp_c_api.h"
#include "keys.h"

namespace bp {

struct RirKeys {
    int rooms = 0, cv_rooms = 0, window = 0;                     // window 0: 2 round(0.004 fs)
    double lo[3] = {3.0, 3.0, 2.5}, hi[3] = {10.0, 8.0, 4.0}, t60[2] = {0.2, 0.8}, margin = 0.5, dist[2] = {0.5, 3.0}, ms = 400.0;
    std::string rooms_out;
    bool any = false;                                            // a key that only means something beside rir_rooms was given
};

// 0: k is not one of the keys; 1: taken; -1: bad value
inline int rir_key(RirKeys &K, const std::string &k, const std::string &v)
{
    auto count = [&v](int *out) { return parse_int(v, 1, 1 << 20, out) ? 1 : -1; };
    if (k == "rir_rooms") return count(&K.rooms);
    if (k == "cv_rir_rooms") return count(&K.cv_rooms);
    int r = 0;
    if (k == "rir_room_lo") r = parse_doubles(v, 3, K.lo) ? 1 : -1;
    else if (k == "rir_room_hi") r = parse_doubles(v, 3, K.hi) ? 1 : -1;
    else if (k == "rir_t60") r = parse_doubles(v, 2, K.t60) ? 1 : -1;
    else if (k == "rir_dist") r = parse_doubles(v, 2, K.dist) ? 1 : -1;
    else if (k == "rir_margin") r = parse_doubles(v, 1, &K.margin) ? 1 : -1;
    else if (k == "rir_ms") r = parse_doubles(v, 1, &K.ms) && K.ms > 0.0 && K.ms <= 1e6 ? 1 : -1;
    else if (k == "rir_window") r = count(&K.window);
    else if (k == "rir_rooms_out") { K.rooms_out = v; r = 1; }
    if (r) K.any = true;
    return r;
}

inline int rir_window_taps(const RirKeys &K, int rate) { return K.window ? K.window : 2 * (int)floor(0.004 * rate + 0.5); }

// n rooms from the seed, each with round(rir_ms rate / 1000) taps; "" or the error
inline std::string rir_draw(const RirKeys &K, unsigned long long seed, int n, int rate, std::vector<bp_rir_room> &rooms, std::vector<int> &len)
{
    bp_rir_range g;
    for (int d = 0; d < 3; ++d) { g.L_lo[d] = K.lo[d]; g.L_hi[d] = K.hi[d]; }
    g.t60_lo = K.t60[0]; g.t60_hi = K.t60[1]; g.margin = K.margin; g.dist_lo = K.dist[0]; g.dist_hi = K.dist[1];
    rooms.assign(n, bp_rir_room());
    if (bp_rir_rooms(seed, n, &g, rooms.data()) != 0) return bp_last_error();
    const double taps = floor(K.ms * rate / 1000.0 + 0.5);
    if (taps < 1.0 || taps > (double)BP_MIX_RIR_MAX_TAPS)
        return "rir_ms: " + std::to_string(K.ms) + " ms are not 1 to " + std::to_string(BP_MIX_RIR_MAX_TAPS) + " taps at " + std::to_string(rate) + " Hz";
    len.assign(n, (int)taps);
    for (int k = 0; k < n; ++k) {
        int order[3];
        int64_t images = 0;
        if (bp_rir_orders(&rooms[k], rate, len[k], rir_window_taps(K, rate), order, &images) != 0) return bp_last_error();
        if (images > BP_RIR_MAX_IMAGES)
            return "rir_rooms: room " + std::to_string(k) + " has " + std::to_string((long long)images) + " images, more than " +
                   std::to_string(BP_RIR_MAX_IMAGES) + " (a shorter rir_ms has fewer)";
    }
    return "";
}

// one text line per room: L, src, mic (3 numbers each), beta (6)
inline std::string rir_write_rooms(const std::string &path, const std::vector<bp_rir_room> &rooms)
{
    FILE *fo = fopen(path.c_str(), "wt");
    if (!fo) return "can not open rooms file: " + path;
    for (const bp_rir_room &r : rooms) {
        const double *part[4] = {r.L, r.src, r.mic, r.beta};
        for (int q = 0; q < 4; ++q)
            for (int i = 0; i < (q < 3 ? 3 : 6); ++i) fprintf(fo, "%.17g%c", part[q][i], q == 3 && i == 5 ? '\n' : ' ');
    }
    fclose(fo);
    return "";
}

// the responses of the rooms, back to back: the one call here that uses the device
inline std::string rir_generate(const RirKeys &K, int device, int rate, const std::vector<bp_rir_room> &rooms, const std::vector<int> &len,
                                std::vector<float> &pcm)
{
    size_t n = 0;
    for (int l : len) n += (size_t)l;
    pcm.assign(n, 0.f);
    if (bp_rir_image(device, rate, rir_window_taps(K, rate), (int)rooms.size(), rooms.data(), len.data(), pcm.data()) != 0) return bp_last_error();
    return "";
}

}  // namespace bp
