#include "wav_io.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace bp {

static uint32_t le32(const unsigned char *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint16_t le16(const unsigned char *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

std::string read_wav(const std::string &path, std::vector<float> &samples, int &sample_rate)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return "can not open wav file: " + path;
    std::vector<unsigned char> b;
    unsigned char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + got);
    fclose(f);
    if (b.size() < 12 || memcmp(&b[0], "RIFF", 4) || memcmp(&b[8], "WAVE", 4)) return path + ": not a RIFF/WAVE file";
    int fmt = -1, channels = 0, bits = 0;
    size_t pos = 12;
    while (pos + 8 <= b.size()) {
        const uint32_t len = le32(&b[pos + 4]);
        const size_t body = pos + 8;
        if (!memcmp(&b[pos], "fmt ", 4)) {
            if (len < 16 || body + len > b.size()) return path + ": truncated fmt chunk";
            fmt = le16(&b[body]); channels = le16(&b[body + 2]); sample_rate = (int)le32(&b[body + 4]); bits = le16(&b[body + 14]);
            if (fmt == 0xFFFE) {                       // WAVE_FORMAT_EXTENSIBLE: the format code opens the sub-format GUID
                if (len < 40) return path + ": truncated fmt chunk";
                fmt = le16(&b[body + 24]);
            }
        } else if (!memcmp(&b[pos], "data", 4)) {
            if (fmt < 0) return path + ": data chunk before fmt chunk";
            if (channels != 1) return path + ": " + std::to_string(channels) + " channels (mono only)";
            if (!((fmt == 1 && bits == 16) || (fmt == 3 && bits == 32)))
                return path + ": format " + std::to_string(fmt) + " with " + std::to_string(bits) + " bits (PCM16 or IEEE float32 only)";
            if (body + len > b.size()) return path + ": truncated data chunk";
            const size_t n = len / (bits / 8);
            samples.resize(n);
            for (size_t i = 0; i < n; ++i) {
                if (fmt == 1) samples[i] = (float)(int16_t)le16(&b[body + 2 * i]);
                else { uint32_t u = le32(&b[body + 4 * i]); float v; memcpy(&v, &u, 4); samples[i] = v * 32768.0f; }
            }
            return std::string();
        }
        pos = body + len + (len & 1);                  // chunks are word aligned
    }
    return path + ": no data chunk";
}

std::string write_wav(const std::string &path, const float *x, size_t n, int sample_rate)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return "can not open output wav file: " + path;
    unsigned char hd[44];
    auto put32 = [&](int at, uint32_t v) { for (int k = 0; k < 4; ++k) hd[at + k] = (unsigned char)(v >> (8 * k)); };
    auto put16 = [&](int at, uint16_t v) { hd[at] = (unsigned char)v; hd[at + 1] = (unsigned char)(v >> 8); };
    memcpy(hd, "RIFF", 4); put32(4, (uint32_t)(36 + 2 * n)); memcpy(hd + 8, "WAVEfmt ", 8);
    put32(16, 16); put16(20, 1); put16(22, 1); put32(24, (uint32_t)sample_rate); put32(28, (uint32_t)sample_rate * 2);
    put16(32, 2); put16(34, 16); memcpy(hd + 36, "data", 4); put32(40, (uint32_t)(2 * n));
    std::vector<unsigned char> b(2 * n);
    for (size_t i = 0; i < n; ++i) {
        const float v = x[i] == x[i] ? nearbyintf(x[i]) : 0.0f;
        const uint16_t u = (uint16_t)(int16_t)(v > 32767.0f ? 32767.0f : v < -32768.0f ? -32768.0f : v);
        b[2 * i] = (unsigned char)u; b[2 * i + 1] = (unsigned char)(u >> 8);
    }
    const bool ok = fwrite(hd, 1, 44, f) == 44 && fwrite(b.data(), 1, b.size(), f) == b.size();
    fclose(f);
    return ok ? std::string() : "write error: " + path;
}

}  // namespace bp
