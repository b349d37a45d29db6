// wav_io.h -- the WAV files of bpfeat / bpenhance: RIFF/WAVE, mono, PCM16 or IEEE float32 (also inside
// WAVE_FORMAT_EXTENSIBLE).  Samples are floats in int16 units: PCM16 as is, float32 x 32768.
#pragma once
#include <string>
#include <vector>

namespace bp {
// returns an empty string on success, else a message that names the file
std::string read_wav(const std::string &path, std::vector<float> &samples, int &sample_rate);
// mono PCM16, samples rounded to nearest and clipped to [-32768, 32767]
std::string write_wav(const std::string &path, const float *samples, size_t n, int sample_rate);
}  // namespace bp
