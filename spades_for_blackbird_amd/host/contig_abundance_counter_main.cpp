// contig_abundance_counter drop-in: the option letters and defaults of the reference tool
// (projects/mts/contig_abundance_counter.cpp:49-87)
//   -k <int> -c <contigs> -n <samples> -m <k-mer multiplicities prefix> -o <output> [-l <length bound = 0>] [-v]
//   (+ -b <bytes> and --device <int>, ours)
// and the flow of Runner::Run (:18-44): for every contig the k-mers found in the profile (ProfileCounter::operator(),
// contig_abundance.cpp:245-284) and, when their share is not below 0.7, one line "<name>\t" + per sample the winsorised
// mean (with -v: mean "\t" variance) + "\t", printed fixed with precision 2.  The first contig shorter than -l ENDS the
// run, as the reference's `break` does.  -m names the <prefix>.kmers / <prefix>.bpr pair kmer_multiplicity_counter
// writes.  A contig keeps every ACGT stretch (SplitOnNs, :172-185): the stretches go to the device as pieces in blocks
// of -b bytes of contig text (bbk_kmerprofile_abundance_pieces); the device returns integers and every float operation
// is done here, one rounding at a time.  A contig of exactly k - 1 characters, on which the reference divides 0 by 0 and
// then fails a VERIFY, gets no line.
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"

using namespace bbkhost;

namespace {

// math::ls (common/math/xmath.h:218-226,300-305): a < b and more than 4 ULPs apart
bool ls(double a, double b) {
    auto biased = [](double x) {
        uint64_t u;
        memcpy(&u, &x, 8);
        return (u >> 63) ? ~u + 1 : (u | (1ull << 63));
    };
    const uint64_t x = biased(a), y = biased(b);
    if (a == a && b == b && (x > y ? x - y : y - x) <= 4) return false;
    return a < b;
}

void usage() {
    printf("Usage: contig_abundance_counter -k <K> -c <contigs path> -n <sample cnt> -m <kmer multiplicities path> "
           "-o <contigs abundance path> [-v] [-l <contig length bound> (default: 0)]\n"
           "       [-b <bytes of contig text per block>] [--device <GPU> (default: 0)]\n");
}

}  // namespace

int main(int argc, char **argv) {
    unsigned long long k = 0, n = 0, min_len = 0, bufsize = 268435456ull;
    unsigned device = 0;
    bool var = false;
    std::string contigs, prefix, outfile;
    Options opt;
    opt.num("-k", "", &k).num("-n", "", &n).num("-l", "", &min_len).num("-b", "", &bufsize, 1ull).num("", "--device", &device)
        .str("-c", "", &contigs).str("-m", "", &prefix).str("-o", "", &outfile).flag("-v", "", &var);
    if (!opt.parse(argc, argv) || !opt.seen("-k") || !opt.seen("-n") || contigs.empty() || prefix.empty() || outfile.empty()) {
        usage();  // GetOptEx (:67-72)
        return 1;
    }
    info("Starting contig abundance counter (MI355X, %s)", bbk_version());
    if (k < 1 || k >= BBK_MAX_K) fatal("k-mer size %llu is out of range [1,%d)", k, BBK_MAX_K);
    if (n < 1 || n > 65535) fatal("sample count %llu is out of range [1,65535]", n);

    Run run;
    Phases &ph = run.ph;
    run.create_ctx(device);
    bbk_ctx *ctx = run.ctx;
    info("Loading kmer index from %s.kmers and profiles from %s.bpr", prefix.c_str(), prefix.c_str());
    const double t0 = now_s();
    bbk_kmerprofile *p = nullptr;
    check(bbk_kmerprofile_load(ctx, prefix.c_str(), (unsigned)k, (unsigned)n, &p), "bbk_kmerprofile_load");
    ph.finish = now_s() - t0;
    info("Kmer index loaded: %llu k-mers, %llu samples", (unsigned long long)bbk_kmerprofile_size(p), n);

    FastxReader rd(contigs);
    if (!rd.is_open()) fatal("cannot open %s", contigs.c_str());
    FILE *out = fopen(outfile.c_str(), "wb");
    if (!out) fatal("cannot open %s for writing", outfile.c_str());
    const unsigned N = (unsigned)n;
    uint64_t n_contigs = 0, n_lines = 0;
    PieceBlock blk;                  // the ACGT stretches of the contigs
    std::vector<std::string> names;  // of the block's contigs
    std::vector<uint64_t> length;    // of the whole contig, other characters included
    std::string text;
    auto flush = [&] {
        const uint64_t nc = blk.sequences(), np = blk.pieces();
        if (nc == 0) return;
        std::vector<uint64_t> hn(nc, 0), hpos(nc, 0), hsum(nc * N, 0), hsq(nc * N, 0);
        if (np > 0) {
            double t1 = now_s();
            bbk_reads *r = nullptr;
            check(bbk_reads_from_ascii(ctx, blk.bases.data(), blk.off.data(), np, &r), "bbk_reads_from_ascii");
            ph.upload += now_s() - t1;
            t1 = now_s();
            check(bbk_kmerprofile_abundance_pieces(ctx, p, r, blk.first_piece.data(), nc, hn.data(), hpos.data(),
                                                   hsum.data(), hsq.data()),
                  "bbk_kmerprofile_abundance_pieces");
            bbk_reads_free(r);
            ph.device += now_s() - t1;
            ++ph.blocks;
        }
        const double t1 = now_s();
        text.clear();
        char buf[64];
        for (uint64_t c = 0; c < nc; ++c) {
            if (hn[c] == 0) continue;  // a share of 0 (or the reference's 0 / 0)
            const uint64_t denom = length[c] - k + 1;  // size_t arithmetic, as s.size() - k_ + 1
            if (ls((double)hn[c] / (double)denom, 0.7)) continue;
            text += names[c];
            text += '\t';
            for (unsigned s = 0; s < N; ++s) {
                // float, one rounded operation per statement (no contraction into a fused multiply-add)
                const volatile float fn = (float)hn[c];
                const volatile float mean = (float)hsum[c * N + s] / fn;
                snprintf(buf, sizeof(buf), "%.2f", (double)mean);
                text += buf;
                if (var) {
                    const volatile float msq = (float)hsq[c * N + s] / fn;
                    const volatile float mm = mean * mean;
                    const volatile float variance = msq - mm;
                    snprintf(buf, sizeof(buf), "\t%.2f", (double)variance);
                    text += buf;
                }
                text += '\t';
            }
            text += '\n';
            ++n_lines;
        }
        if (!text.empty() && fwrite(text.data(), 1, text.size(), out) != text.size())
            fatal("writing %s failed", outfile.c_str());
        ph.write += now_s() - t1;
        blk = PieceBlock();
        names.clear();
        length.clear();
    };
    const double tl = now_s();
    std::string name, seq, qual;
    while (rd.next_record(name, seq, qual)) {  // upper-cased by the reader; is_nucl takes either case
        if (seq.size() < min_len) break;
        blk.add(seq, [](char ch) { return ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T'; });
        names.push_back(name);
        length.push_back(seq.size());
        ++n_contigs;
        if (blk.bases.size() >= bufsize) flush();
    }
    flush();
    ph.parse = now_s() - tl - ph.upload - ph.device - ph.write;
    if (fclose(out) != 0) fatal("writing %s failed", outfile.c_str());
    info("%llu contigs analysed, %llu abundance lines written to %s", (unsigned long long)n_contigs,
         (unsigned long long)n_lines, outfile.c_str());
    bbk_kmerprofile_free(p);
    run.done("contig_abundance_counter");
}
