// pfile_writer.h -- ICSI Pfile output (the format PfileReader reads): a 32768-byte text header, one record per frame
// (sentence id, frame id, features; big-endian 32-bit words), then the sentence table (num_sentences + 1 cumulative frame
// offsets).  Shared by bpforward (enhanced LPS) and bpfeat (noisy / clean LPS for training); header-only, so each tool links it
// without another source file.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace bp {
class PfileWriter {
public:
    // n_sent sentences of n_features features; false when the file cannot be created
    inline bool open(const std::string &path, int n_sent, int n_features);
    // one record; a sentence id outside [0, n_sent) is written but not counted in the sentence table
    inline void add(int sent, int frame, const float *feat);
    inline void close();                // sentence table + header
private:
    FILE *fo_ = nullptr;
    int nf_ = 0;
    unsigned total_ = 0;
    std::vector<uint32_t> per_sent_, rec_;
};

inline uint32_t pfile_be32(uint32_t v) { return __builtin_bswap32(v); }
const size_t PFILE_HEADER_BYTES = 32768;

bool PfileWriter::open(const std::string &path, int n_sent, int n_features)
{
    fo_ = fopen(path.c_str(), "wb");
    if (!fo_) return false;
    nf_ = n_features; total_ = 0;
    per_sent_.assign((size_t)n_sent, 0u);
    rec_.resize(2 + (size_t)n_features);
    std::vector<char> header(PFILE_HEADER_BYTES, 0);
    fwrite(header.data(), 1, header.size(), fo_);        // rewritten by close() with the counts
    return true;
}

void PfileWriter::add(int sent, int frame, const float *feat)
{
    rec_[0] = pfile_be32((uint32_t)sent); rec_[1] = pfile_be32((uint32_t)frame);
    for (int k = 0; k < nf_; ++k) { uint32_t u; memcpy(&u, &feat[k], 4); rec_[2 + k] = pfile_be32(u); }
    fwrite(rec_.data(), 4, rec_.size(), fo_);
    if (sent >= 0 && sent < (int)per_sent_.size()) per_sent_[sent]++;
    ++total_;
}

void PfileWriter::close()
{
    uint32_t cum = 0, v = pfile_be32(0);
    fwrite(&v, 4, 1, fo_);
    for (uint32_t n : per_sent_) { cum += n; v = pfile_be32(cum); fwrite(&v, 4, 1, fo_); }
    std::vector<char> header(PFILE_HEADER_BYTES, 0);
    snprintf(header.data(), header.size(), "-pfile_header version 0 size 32768\n-num_sentences %d\n-num_frames %u\n-first_feature_column 2\n-num_features %d\n-end\n",
             (int)per_sent_.size(), total_, nf_);
    fseek(fo_, 0, SEEK_SET);
    fwrite(header.data(), 1, header.size(), fo_);
    fclose(fo_);
    fo_ = nullptr;
}

}  // namespace bp
