// hammer_run.hpp -- one iteration of BayesHammer on the engine (projects/hammer/main.cpp:118-252): count, cluster,
// statistics, subcluster, expand, correct, over the input files of a dataset, parameterised by a plain struct.  Two tools
// are this sequence: spades-kmerdata (kmerdata_main.cpp: one iteration, every step optional, the intermediate files
// always written) and spades-hammer (hammer_main.cpp: general_max_iterations iterations from a config.info).
#pragma once

#include <sys/stat.h>

#include <cerrno>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "common.hpp"

namespace bbkhost {

// An input file as CorrectAllReads sees it: its library, its number in the library (pairs first, then merged, then single
// files: hammer_tools.cpp:233-268) and the list of the corrected library its output joins
struct InFile {
    std::string path;
    size_t ilib = 0, iread = 0;
    int kind = LIB_SINGLE;  // LIB_LEFT / LIB_RIGHT: a mate file of a pair; LIB_MERGED; anything else counts as single
};
// What is read together: one single-read file, or the two files of a pair in step
struct Group {
    size_t f0 = 0;
    long f1 = -1;  // the right file of a pair, or -1
};

// One block of records of one input file, as parsed, and its prepared batch on the device (bbk_hreads: the trims, the
// stretches and the candidates of every record).  A resident block keeps the batch, the names, the qualities and the
// offsets for the later passes and lets the bases go.  The block of a left file owns the block of the same records of the
// right file.
struct Block {
    size_t group = 0, file = 0;
    std::string bases, quals;  // quals: the offset subtracted
    std::vector<uint64_t> offsets{0};
    std::string names;  // back to back
    std::vector<uint64_t> name_off{0};
    bbk_hreads *hr = nullptr;
    bool resident = false;
    bool device = false;  // parsed on the device (--device-parse): the batch holds the records and their names, the host nothing
    std::unique_ptr<Block> mate;
    uint64_t size() const { return device ? bbk_hreads_size(hr) : offsets.size() - 1; }
    uint64_t total() const { return device ? bbk_hreads_bases(hr) : offsets.back(); }
    ~Block() { bbk_hreads_free(hr); }
};

// The text of one file on its way to the device (--device-parse): a reused buffer that holds the text behind the last
// record taken, and the index of that text.
struct TextFeed {
    std::string path;
    gzFile fp = nullptr;
    std::vector<char> buf;
    size_t have = 0, want = 0;  // bytes in buf; bytes a chunk is read up to
    uint64_t file_off = 0;      // where buf[0] is in the (uncompressed) file
    bool eof = false;
    bbk_fastq_input *in = nullptr;
    uint64_t next = 0, usable = 0;  // the first record of the index not taken yet; its records before the verdict
    bool verdict = false;

    TextFeed() = default;
    TextFeed(const TextFeed &) = delete;
    TextFeed &operator=(const TextFeed &) = delete;
    ~TextFeed() {
        bbk_fastq_input_free(in);
        if (fp) gzclose(fp);
    }
    void open(const std::string &p, size_t chunk) {
        path = p;
        fp = gzopen(p.c_str(), "r");
        if (!fp) fatal("cannot open %s", p.c_str());
        gzbuffer(fp, 1 << 20);
        want = chunk;
    }
    uint64_t avail() const { return usable - next; }
    bool can_extend() const { return !eof && !verdict; }  // more text would give more usable records
    uint64_t offset_of_next() const { return file_off + bbk_fastq_input_text_end(in, next); }
    // Drops the text of the records taken, reads on (a chunk that did not hold a block grows) and indexes what is there
    void advance(bbk_ctx *ctx, int qvoffset) {
        if (in) {
            const size_t consumed = (size_t)bbk_fastq_input_text_end(in, next);
            memmove(buf.data(), buf.data() + consumed, have - consumed);
            have -= consumed;
            file_off += consumed;
            bbk_fastq_input_free(in);
            in = nullptr;
            if (have >= want / 2) want *= 2;
        }
        if (buf.size() < want) buf.resize(want);
        while (have < want && !eof) {
            const int n = gzread(fp, buf.data() + have, (unsigned)std::min<size_t>(want - have, 1u << 30));
            if (n < 0) fatal("cannot read %s", path.c_str());
            if (n == 0) eof = true;
            have += (size_t)n;
        }
        check(bbk_fastq_input_from_host(ctx, buf.data(), have, eof ? 1 : 0, qvoffset, &in), "bbk_fastq_input_from_host");
        uint64_t record = 0;
        verdict = bbk_fastq_input_verdict(in, &record, nullptr, nullptr) != 0;
        usable = verdict ? record : bbk_fastq_input_records(in);
        next = 0;
    }
};

// The records of all groups as prepared blocks, in group order, once per pass.  A block holds the records of one file up
// to -b bases -- of a pair: up to the record at which either file reaches -b, the same records of both -- so every pass
// and every --resident-bytes sees the same blocks.  The blocks of the first pass stay on the device while their bases and
// qualities fit --resident-bytes; the later passes take those as they are and parse the files again only for the blocks
// behind them.
class ReadSource {
public:
    ReadSource(bbk_ctx *ctx, const std::vector<InFile> &files, const std::vector<Group> &groups, unsigned k, int qvoffset,
               int trim_quality, size_t block_bytes, uint64_t resident_bytes, bool device_parse, size_t parse_chunk)
        : ctx_(ctx), files_(files), groups_(groups), k_(k), qvoffset_(qvoffset), trim_quality_(trim_quality),
          block_bytes_(block_bytes), budget_(resident_bytes), keeping_(resident_bytes != 0), kept_in_group_(groups.size(), 0),
          whole_group_(groups.size(), false), device_parse_(device_parse), parse_chunk_(parse_chunk), resume_(groups.size()) {}

    // fn(block) for the block of every group's first file (its mate, if any, hangs on it); returns the number of records
    template <class F>
    uint64_t each_group(bool announce, F fn) {
        uint64_t records = 0;
        for (const auto &b : resident_) {
            fn(*b);
            records += b->size() + (b->mate ? b->mate->size() : 0);
        }
        for (size_t g = 0; g < groups_.size(); ++g) {
            if (whole_group_[g]) continue;
            if (announce) {
                info("Processing %s", files_[groups_[g].f0].path.c_str());
                if (groups_[g].f1 >= 0) info("Processing %s", files_[(size_t)groups_[g].f1].path.c_str());
            }
            records += parse(g, fn);
        }
        keeping_ = false;
        return records;
    }
    // fn(block) for every block, a left block before its mate
    template <class F>
    uint64_t each(bool announce, F fn) {
        return each_group(announce, [&](const Block &b) {
            fn(b);
            if (b.mate) fn(*b.mate);
        });
    }

    void clear() { resident_.clear(); }  // the resident blocks leave the device

private:
    void take(Block &b, size_t f, uint64_t record, const std::string &name, const std::string &seq, std::string &qual) {
        if (qual.size() != seq.size())
            fatal("%s: record %llu (%s) has no quality string: the statistics need FASTQ input", files_[f].path.c_str(),
                  (unsigned long long)record, name.c_str());
        for (char &c : qual) {
            const int q = (unsigned char)c - qvoffset_;
            if (q < 0 || q > 93)
                fatal("%s: record %llu (%s): quality character '%c' is outside [0, 93] at offset %d", files_[f].path.c_str(),
                      (unsigned long long)record, name.c_str(), c, qvoffset_);
            c = (char)q;
        }
        b.bases += seq;
        b.quals += qual;
        b.offsets.push_back(b.bases.size());
        b.names += name;
        b.name_off.push_back(b.names.size());
    }
    void prepare(Block &b, size_t g, size_t f) {
        b.group = g;
        b.file = f;
        check(bbk_hreads_from_host(ctx_, b.bases.data(), reinterpret_cast<const uint8_t *>(b.quals.data()), b.offsets.data(), b.size(),
                                   k_, trim_quality_, &b.hr),
              "bbk_hreads_from_host");
    }

    // Where the serial reader takes a group over from the device parser
    struct Resume {
        bool known = false;
        uint64_t off[2] = {0, 0}, in_file = 0, block_no = 0;
    };

    std::unique_ptr<Block> fresh(bool paired) const {
        std::unique_ptr<Block> b(new Block);
        if (paired) b->mate.reset(new Block);
        return b;
    }
    // Block number block_no of group g is complete: handed to fn unless it is resident and has been handed out already,
    // then kept while the budget lasts
    template <class F>
    void hand_out(size_t g, std::unique_ptr<Block> &b, uint64_t &block_no, uint64_t &records, F &fn) {
        const bool paired = groups_[g].f1 >= 0;
        if (block_no++ < kept_in_group_[g]) return;  // the blocks before are resident and have been handed out
        const size_t f0 = groups_[g].f0, f1 = paired ? (size_t)groups_[g].f1 : f0;
        if (!b->device) {
            prepare(*b, g, f0);
            if (paired) prepare(*b->mate, g, f1);
        }
        fn(*b);
        const uint64_t held = 2 * (b->total() + (paired ? b->mate->total() : 0));
        records += b->size() + (paired ? b->mate->size() : 0);
        if (keeping_ && held_ + held <= budget_) {
            held_ += held;
            b->resident = true;
            std::string().swap(b->bases);
            if (paired) {
                b->mate->resident = true;
                std::string().swap(b->mate->bases);
            }
            ++kept_in_group_[g];
            resident_.push_back(std::move(b));
        } else {
            keeping_ = false;  // the resident blocks are a prefix of all blocks
        }
    }

    template <class F>
    uint64_t parse(size_t g, F &fn) {
        return device_parse_ ? parse_device(g, fn) : parse_host(g, fn, Resume());
    }

    // The serial reader over the group, from the start or from where the device parser left it
    template <class F>
    uint64_t parse_host(size_t g, F &fn, const Resume &from) {
        const size_t f0 = groups_[g].f0;
        const bool paired = groups_[g].f1 >= 0;
        const size_t f1 = paired ? (size_t)groups_[g].f1 : f0;
        FastxReader rl(files_[f0].path);
        if (!rl.is_open()) fatal("cannot open %s", files_[f0].path.c_str());
        std::unique_ptr<FastxReader> rr;
        if (paired) {
            rr.reset(new FastxReader(files_[f1].path));
            if (!rr->is_open()) fatal("cannot open %s", files_[f1].path.c_str());
        }
        if (from.known && (!rl.seek(from.off[0]) || (paired && !rr->seek(from.off[1]))))
            fatal("cannot position %s at the record the serial reader takes over from", files_[f0].path.c_str());
        std::unique_ptr<Block> b = fresh(paired);
        std::string name, seq, qual, name2, seq2, qual2;
        uint64_t records = 0, in_file = from.in_file, block_no = from.block_no;
        for (;;) {
            const bool more = rl.next_record(name, seq, qual);
            if (paired && rr->next_record(name2, seq2, qual2) != more)  // hammer_tools.cpp:190-191
                fatal("Pair of read files %s and %s contain unequal amount of reads", files_[f0].path.c_str(), files_[f1].path.c_str());
            if (!more) break;
            take(*b, f0, in_file, name, seq, qual);
            if (paired) take(*b->mate, f1, in_file, name2, seq2, qual2);
            ++in_file;
            if (b->bases.size() >= block_bytes_ || (paired && b->mate->bases.size() >= block_bytes_)) {
                hand_out(g, b, block_no, records, fn);
                b = fresh(paired);
            }
        }
        if (b->size()) hand_out(g, b, block_no, records, fn);
        if (keeping_) whole_group_[g] = true;
        return records;
    }

    // The same blocks cut from text that is indexed on the device.  A block is complete when a side has a record at which
    // its bases reach -b BEFORE its last usable record (the block rule stops there: more text cannot change it); a side
    // whose usable records run out first reads on, and where it cannot -- a verdict, or the end of the file -- the
    // serial reader takes over at the block's first record, or the group ends.
    template <class F>
    uint64_t parse_device(size_t g, F &fn) {
        const bool paired = groups_[g].f1 >= 0;
        const int ns = paired ? 2 : 1;
        const size_t f[2] = {groups_[g].f0, paired ? (size_t)groups_[g].f1 : groups_[g].f0};
        Resume &rs = resume_[g];
        TextFeed fd[2];
        uint64_t records = 0, in_file = 0, block_no = 0;
        for (int s = 0; s < ns; ++s) fd[s].open(files_[f[s]].path, parse_chunk_);
        auto unequal = [&] {
            fatal("Pair of read files %s and %s contain unequal amount of reads", files_[f[0]].path.c_str(), files_[f[1]].path.c_str());
        };
        for (;;) {
            if (rs.known && block_no == rs.block_no) return records + parse_host(g, fn, rs);
            for (int s = 0; s < ns; ++s)
                if (!fd[s].in) fd[s].advance(ctx_, qvoffset_);
            uint64_t c = ~0ull;  // the records of the block, when a side closes it
            for (int s = 0; s < ns; ++s) {
                const uint64_t cs = bbk_fastq_input_records_within(fd[s].in, fd[s].next, block_bytes_);
                if (cs < fd[s].avail()) c = std::min(c, cs);
            }
            bool last = false, again = false, give_up = false;
            if (c != ~0ull) {
                for (int s = 0; s < ns; ++s) {
                    if (fd[s].avail() >= c) continue;
                    if (fd[s].can_extend()) again = true, fd[s].advance(ctx_, qvoffset_);
                    else if (fd[s].verdict) give_up = true;
                    else unequal();  // the file ends inside a block the other file completes
                }
            } else {
                for (int s = 0; s < ns; ++s) give_up = give_up || fd[s].verdict;
                for (int s = 0; s < ns && !give_up; ++s)
                    if (fd[s].can_extend()) again = true, fd[s].advance(ctx_, qvoffset_);
                if (!give_up && !again) {  // every file is at its end: what is left is the last block
                    if (paired && fd[0].avail() != fd[1].avail()) unequal();
                    c = fd[0].avail();
                    last = true;
                }
            }
            if (give_up) {
                rs.known = true;
                for (int s = 0; s < ns; ++s) rs.off[s] = fd[s].offset_of_next();
                rs.in_file = in_file;
                rs.block_no = block_no;
                info("%s: not in the four-line form behind record %llu: the serial reader goes on from there",
                     files_[f[0]].path.c_str(), (unsigned long long)in_file);
                continue;
            }
            if (again) continue;
            if (c) {
                std::unique_ptr<Block> b = fresh(paired);
                if (block_no >= kept_in_group_[g]) {
                    Block *side[2] = {b.get(), b->mate.get()};
                    for (int s = 0; s < ns; ++s) {
                        side[s]->device = true;
                        side[s]->group = g;
                        side[s]->file = f[s];
                        check(bbk_hreads_from_fastq_input(fd[s].in, fd[s].next, c, k_, trim_quality_, &side[s]->hr),
                              "bbk_hreads_from_fastq_input");
                    }
                }
                hand_out(g, b, block_no, records, fn);
                for (int s = 0; s < ns; ++s) fd[s].next += c;
                in_file += c;
            }
            if (last) break;
        }
        if (keeping_) whole_group_[g] = true;
        return records;
    }

    bbk_ctx *ctx_;
    const std::vector<InFile> &files_;
    const std::vector<Group> &groups_;
    unsigned k_;
    int qvoffset_, trim_quality_;
    size_t block_bytes_;
    uint64_t budget_, held_ = 0;
    bool keeping_;
    std::vector<std::unique_ptr<Block>> resident_;
    std::vector<uint64_t> kept_in_group_;  // resident blocks of every group: its first ones
    std::vector<bool> whole_group_;        // every block of the group is resident
    bool device_parse_;
    size_t parse_chunk_;
    std::vector<Resume> resume_;  // per group: found in the first pass that gets there, used by every later one
};

// fs::basename (common/utils/filesystem/path_helper.cpp:104-113): no directory, no last extension
inline std::string ref_basename(const std::string &path) {
    const size_t slash = path.find_last_of('/'), after = slash == std::string::npos ? 0 : slash + 1;
    size_t dot = path.find_last_of('.');
    if (dot != std::string::npos && dot < after) dot = std::string::npos;
    return path.substr(after, dot == std::string::npos ? std::string::npos : dot - after);
}
// getReadsFilename (hammer_tools.cpp:53-59): the iteration number as setw(2) with setfill('0')
inline std::string ref_reads_filename(const std::string &dir, const std::string &fname, unsigned iteration, const std::string &suffix) {
    char ii[16];
    snprintf(ii, sizeof(ii), "%02u", iteration);
    return dir + "/" + ref_basename(fname) + "." + ii + "." + suffix;
}
inline std::string largest_prefix(const std::string &a, const std::string &b) {  // hammer_tools.cpp:195-204
    size_t i = 0;
    while (i < a.size() && i < b.size() && a[i] == b[i]) ++i;
    return a.substr(0, i);
}

// CorrectAllReads' loop over the read files (hammer_tools.cpp:218-277) as a thin loop over the blocks: a block -- with its
// mate, CorrectPairedReadFiles (:144-193), without, CorrectReadFile (:107-142) -- is corrected, printed on the device and
// every stream of the text appended to the file of that stream
struct CorrectedWriter {
    const std::vector<InFile> &files;
    const std::vector<Group> &groups;
    const std::string &prefix, &out_dir;  // out_dir empty: <prefix>.<i>.* names
    bbk_ctx *ctx;
    bbk_corrector *cor;
    int qvoffset;
    bool tags;
    unsigned iteration;  // Globals::iteration_no in the names under out_dir
    std::vector<DatasetLib> &outlibs;
    size_t open_group = 0;
    bool is_open = false;
    std::string path[5];
    unsigned buffer_no = 0;

    // the files of group g, and of every group before it that had no block: created empty, appended to block by block
    void open_until(size_t g) {
        while (!is_open || open_group < g) {
            if (is_open) ++open_group;
            if (open_group >= groups.size()) return;
            const Group &G = groups[open_group];
            const InFile &l = files[G.f0];
            int n = 2;
            auto names = [&](const InFile &f, size_t index, std::string &cor_path, std::string &bad_path) {
                const std::string usuffix = std::to_string(f.ilib) + "_" + std::to_string(f.iread) + ".cor.fastq";
                cor_path = out_dir.empty() ? prefix + "." + std::to_string(index) + ".cor.fastq" : ref_reads_filename(out_dir, f.path, iteration, usuffix);
                bad_path = out_dir.empty() ? prefix + "." + std::to_string(index) + ".bad.fastq" : ref_reads_filename(out_dir, f.path, iteration, "bad.fastq");
            };
            if (G.f1 < 0) {
                info(l.kind == LIB_MERGED ? "Correcting merged reads: %s" : "Correcting single reads: %s", l.path.c_str());
                names(l, G.f0, path[0], path[1]);
                outlibs[l.ilib].v[l.kind == LIB_MERGED ? LIB_MERGED : LIB_SINGLE].push_back(path[0]);
            } else {
                const InFile &r = files[(size_t)G.f1];
                info("Correcting pair of reads: %s and %s", l.path.c_str(), r.path.c_str());
                names(l, G.f0, path[0], path[3]);
                names(r, (size_t)G.f1, path[1], path[4]);
                const std::string usuffix = std::to_string(l.ilib) + "_" + std::to_string(l.iread) + ".cor.fastq";
                path[2] = out_dir.empty() ? prefix + "." + std::to_string(G.f0) + ".unpaired.fastq"
                                          : ref_reads_filename(out_dir, largest_prefix(l.path, r.path) + "_unpaired.fastq", iteration, usuffix);
                outlibs[l.ilib].v[LIB_LEFT].push_back(path[0]);
                outlibs[l.ilib].v[LIB_RIGHT].push_back(path[1]);
                outlibs[l.ilib].v[LIB_SINGLE].push_back(path[2]);
                n = 5;
            }
            for (int s = 0; s < n; ++s) {
                FILE *f = fopen(path[s].c_str(), "wb");
                if (!f || fclose(f) != 0) fatal("cannot open %s for writing", path[s].c_str());
            }
            is_open = true;
            buffer_no = 0;
        }
    }
    void finish() { open_until(groups.empty() ? 0 : groups.size() - 1); }
    void operator()(const Block &b) {
        open_until(b.group);
        const Block *m = b.mate.get();
        info("Prepared batch %u of %llu reads.", buffer_no, (unsigned long long)b.size());
        bbk_corrected *left = nullptr, *right = nullptr;
        check(bbk_corrector_correct_resident(cor, b.hr, &left), "bbk_corrector_correct_resident");
        if (m) check(bbk_corrector_correct_resident(cor, m->hr, &right), "bbk_corrector_correct_resident");
        info("Processed batch %u", buffer_no);
        bbk_fastq_text *text = nullptr;
        if (b.device)  // the names are the batch's own
            check(bbk_corrected_print_resident(left, right, qvoffset, tags ? 1 : 0, &text), "bbk_corrected_print_resident");
        else
            check(bbk_corrected_print(left, right, b.names.data(), b.name_off.data(), m ? m->names.data() : nullptr,
                                      m ? m->name_off.data() : nullptr, qvoffset, tags ? 1 : 0, &text),
                  "bbk_corrected_print");
        for (int s = 0; s < bbk_fastq_text_streams(text); ++s)
            if (bbk_fastq_text_size(text, s)) check(bbk_fastq_text_write(ctx, text, s, path[s].c_str(), 1), "bbk_fastq_text_write");
        bbk_fastq_text_free(text);
        bbk_corrected_free(right);
        bbk_corrected_free(left);
        info("Written batch %u", buffer_no);
        ++buffer_no;
    }
};

// The libraries of a run: the positional files as one library, or those of the dataset description
inline std::vector<DatasetLib> input_libs(const std::vector<std::string> &input, const std::string &dataset, bool paired) {
    std::vector<DatasetLib> libs;
    if (dataset.empty()) {
        libs.emplace_back();
        if (paired) {
            if (input.size() % 2) fatal("--paired: %zu input files: a pair is a left and a right file", input.size());
            for (size_t i = 0; i < input.size(); ++i) libs[0].v[i % 2 ? LIB_RIGHT : LIB_LEFT].push_back(input[i]);
        } else {
            libs[0].v[LIB_SINGLE] = input;
        }
    } else {
        std::string err;
        if (!load_dataset_libs(dataset, libs, err)) fatal("%s", err.c_str());
    }
    return libs;
}

// The input files in the order the passes take them, what is read together, and the corrected libraries to be filled
inline void plan_input(const std::vector<DatasetLib> &libs, bool paired, std::vector<InFile> &files, std::vector<Group> &groups,
                       std::vector<DatasetLib> &outlibs) {
    for (size_t ilib = 0; ilib < libs.size(); ++ilib) {
        const DatasetLib &lib = libs[ilib];
        outlibs.emplace_back();
        outlibs.back().type = lib.type;
        outlibs.back().orientation = lib.orientation;
        size_t iread = 0;
        auto single = [&](const std::string &p, int kind) {
            files.push_back({p, ilib, iread++, kind});
            groups.push_back({files.size() - 1, -1});
        };
        if (paired) {
            if (!lib.v[LIB_INTERLACED].empty())
                fatal("--paired: library %zu has interlaced reads (%s): interlaced libraries are not supported", ilib,
                      lib.v[LIB_INTERLACED][0].c_str());
            if (lib.v[LIB_LEFT].size() != lib.v[LIB_RIGHT].size())
                fatal("--paired: library %zu has %zu left and %zu right read files", ilib, lib.v[LIB_LEFT].size(), lib.v[LIB_RIGHT].size());
            for (size_t i = 0; i < lib.v[LIB_LEFT].size(); ++i, ++iread) {
                files.push_back({lib.v[LIB_LEFT][i], ilib, iread, LIB_LEFT});
                files.push_back({lib.v[LIB_RIGHT][i], ilib, iread, LIB_RIGHT});
                groups.push_back({files.size() - 2, (long)files.size() - 1});
            }
        } else {  // every file a single-read file, in the order of the dataset's keys
            for (int kind : {LIB_LEFT, LIB_RIGHT, LIB_INTERLACED})
                for (const std::string &p : lib.v[kind]) single(p, LIB_SINGLE);
        }
        for (const std::string &p : lib.v[LIB_MERGED]) single(p, LIB_MERGED);
        for (const std::string &p : lib.v[LIB_SINGLE]) single(p, LIB_SINGLE);
    }
}

// corrected.yaml, the description of the corrected libraries (main.cpp:254-256)
inline void save_corrected_yaml(const std::string &out_dir, const std::vector<DatasetLib> &libs) {
    const std::string yaml = out_dir + "/corrected.yaml";
    info("Saving corrected dataset description to %s", yaml.c_str());
    if (!save_dataset_yaml(yaml, libs)) fatal("cannot write %s", yaml.c_str());
}

// The solid k-mer expansion in snapshot rounds (main.cpp:194-222): the expander with the expanded good bits, stored in sc
inline bbk_expander *expand_solid(bbk_ctx *ctx, const bbk_kmerset *set, bbk_subclusters *sc, ReadSource &src,
                                  unsigned max_iterations, unsigned long long min_changed) {
    bbk_expander *ex = nullptr;
    check(bbk_expander_from_subclusters(ctx, set, sc, &ex), "bbk_expander_from_subclusters");
    info("Starting solid k-mers expansion in snapshot rounds.");
    for (unsigned iter = 0; iter < max_iterations; ++iter) {
        check(bbk_expander_round_begin(ex), "bbk_expander_round_begin");
        src.each(false, [&](const Block &b) {
            const bbk_reads *r = nullptr;
            check(bbk_hreads_candidate_view(b.hr, &r), "bbk_hreads_candidate_view");
            check(bbk_expander_push(ex, r, nullptr), "bbk_expander_push");
            // push does not wait, and a block that is not resident goes now
            if (!b.resident) check(bbk_ctx_synchronize(ctx), "bbk_ctx_synchronize");
        });
        uint64_t changed = 0;
        check(bbk_expander_round_end(ex, &changed), "bbk_expander_round_end");
        info("Solid k-mers iteration %u produced %llu new k-mers.", iter, (unsigned long long)changed);
        if (changed < min_changed) break;
    }
    info("Solid k-mers finalized");
    check(bbk_expander_store(ex, sc), "bbk_expander_store");
    return ex;
}

// CorrectAllReads (hammer_tools.cpp:218-277): every block through w, which gets its corrector here; then the counters and,
// with save_yaml under --output-dir, corrected.yaml (main.cpp:254-256).  Returns changedReads.
inline uint64_t correct_reads(const bbk_kmerset *set, const bbk_expander *ex, ReadSource &src, CorrectedWriter &w, bool save_yaml) {
    check(bbk_corrector_from_expander(w.ctx, set, ex, &w.cor), "bbk_corrector_from_expander");
    info("Starting read correction.");
    src.each_group(false, std::ref(w));
    w.finish();
    uint64_t cs[5];
    check(bbk_corrector_stats(w.cor, cs), "bbk_corrector_stats");
    info("Correction done. Changed %llu bases in %llu reads.", (unsigned long long)cs[1], (unsigned long long)cs[0]);
    info("Failed to correct %llu bases out of %llu.", (unsigned long long)cs[2], (unsigned long long)cs[3]);
    info("  Searches corrected on the host: %llu", (unsigned long long)cs[4]);
    if (save_yaml && !w.out_dir.empty()) save_corrected_yaml(w.out_dir, w.outlibs);
    bbk_corrector_free(w.cor);
    return cs[0];
}

// The report of KMerClustering::process (kmer_cluster.cpp:650-658)
inline void report_subclusters(bbk_ctx *ctx, const bbk_subclusters *sc) {
    uint64_t st[9], errs[16];
    check(bbk_subclusters_export(ctx, sc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, errs, st), "bbk_subclusters_export");
    const uint64_t gsingl = st[0], tsingl = st[1], tcsingl = st[2], gcsingl = st[3], tcls = st[4], gcls = st[5],
                   tkmers = st[6], tncls = st[7], newkmers = st[8];
    info("Subclustering done. Total %llu non-read kmers were generated.", (unsigned long long)newkmers);
    info("Subclustering statistics:");
    info("  Total singleton hamming clusters: %llu. Among them %llu (%g%%) are good", (unsigned long long)tsingl,
         (unsigned long long)gsingl, 100.0 * (double)gsingl / (double)tsingl);
    info("  Total singleton subclusters: %llu. Among them %llu (%g%%) are good", (unsigned long long)tcsingl,
         (unsigned long long)gcsingl, 100.0 * (double)gcsingl / (double)tcsingl);
    info("  Total non-singleton subcluster centers: %llu. Among them %llu (%g%%) are good", (unsigned long long)tcls,
         (unsigned long long)gcls, 100.0 * (double)gcls / (double)tcls);
    info("  Average size of non-trivial subcluster: %g kmers", 1.0 * (double)tkmers / (double)tcls);
    info("  Average number of sub-clusters per non-singleton cluster: %g", 1.0 * (double)(tcsingl + tcls) / (double)tncls);
    info("  Total solid k-mers: %llu", (unsigned long long)(gsingl + gcsingl + gcls));
    std::string m;
    for (int r = 0; r < 4; ++r) {
        uint64_t row = 0;
        for (int c = 0; c < 4; ++c) row += errs[4 * r + c];
        for (int c = 0; c < 4; ++c) {
            char b[64];
            snprintf(b, sizeof(b), "%s%g", c ? "," : "", (double)errs[4 * r + c] / (double)row);
            m += b;
        }
        m += r < 3 ? ")," : ")";
        if (r < 3) m += "(";
    }
    info("  Substitution probabilities: [4,4]((%s)", m.c_str());
    info("  K-mers subclustered on the host: %llu", (unsigned long long)bbk_subclusters_host_kmers(sc));
}

// What one iteration is made of.  The defaults are those of configs/hammer/config.info and of spades-kmerdata's options.
struct HammerParams {
    unsigned K = 21;
    bbk_subcluster_params sp = {0.995, 0.9, 0.98, 1};
    unsigned expand_max_iterations = 25;
    unsigned long long expand_min_changed = 10;  // main.cpp:219
    int qvoffset = 33, trim_quality = 4;
    size_t block_bytes = 536870912ull, parse_chunk = 67108864ull;
    uint64_t resident_bytes = 0;
    bool device_parse = false;
    bool cluster = false, subcluster = false, expand = false, correct = false;  // every step implies the ones before it
    bool correct_stats = false;
    unsigned iteration = 0;          // Globals::iteration_no: in the names of the corrected reads under out_dir
    bool filter_singletons = false;  // count_filter_singletons: pass 1 keeps the k-mers of multiplicity 2 and more
    std::string out_dir;             // the corrected reads under the reference's names; empty: <prefix>.<i>.* names
    std::string prefix;              // the intermediate files (.kmers, .kmstat, .hamming*, .subclusters*, .newkmers); empty: none
    bool save_yaml = true;           // with out_dir: corrected.yaml behind the correction
};

// One iteration of main.cpp:118-252 over the planned input (plan_input): returns changedReads of the correction (0 without
// one); outlibs receives the corrected libraries
inline uint64_t run_hammer_iteration(bbk_ctx *ctx, Phases &ph, const HammerParams &p, const std::vector<InFile> &files,
                                     const std::vector<Group> &groups, std::vector<DatasetLib> &outlibs) {
    // pass 1: the set
    bbk_counter *counter = nullptr;
    check(bbk_count_begin(ctx, p.K, BBK_BOTH_STRANDS | (p.filter_singletons ? BBK_WITH_COUNTS : 0u), &counter), "bbk_count_begin");
    uint64_t stretches = 0;
    double t0 = now_s();
    ReadSource src(ctx, files, groups, p.K, p.qvoffset, p.trim_quality, p.block_bytes, p.resident_bytes, p.device_parse,
                   p.parse_chunk);
    const uint64_t records = src.each(true, [&](const Block &b) {
        const bbk_reads *r = nullptr;
        check(bbk_hreads_stretch_view(b.hr, &r, nullptr), "bbk_hreads_stretch_view");
        check(bbk_count_push_reads(counter, r), "bbk_count_push_reads");
        stretches += bbk_hreads_kmer_stretches(b.hr);
        ++ph.blocks;
    });
    info("Total %llu reads processed, %llu stretches of valid k-mers", (unsigned long long)records,
         (unsigned long long)stretches);
    bbk_kmerset *set = nullptr;
    if (p.filter_singletons) {  // KMerDataCounter::BuildKMerIndex with count_filter_singletons (kmer_data.cpp:280-335), exact
        uint64_t dropped = 0;
        check(bbk_count_finish_min_count(counter, 2, &set, &dropped), "bbk_count_finish_min_count");
        info("Singleton filter: %llu k-mers of multiplicity 1 dropped.", (unsigned long long)dropped);
    } else {
        check(bbk_count_finish(counter, &set), "bbk_count_finish");
    }
    const uint64_t n = bbk_kmerset_size(set);
    info("K-mer counting done. There are %llu kmers in total.", (unsigned long long)n);

    bbk_hamclusters *hc = nullptr;
    if (p.cluster) check(bbk_kmerset_hamming_clusters(ctx, set, 1, 0, 0, &hc), "bbk_kmerset_hamming_clusters");

    // pass 2: the statistics
    info("Collecting K-mer information");
    bbk_kmerstats *ks = nullptr;
    check(bbk_kmerstats_begin(ctx, set, &ks), "bbk_kmerstats_begin");
    src.each(false, [&](const Block &b) {
        const bbk_reads *r = nullptr;
        const bbk_quals *q = nullptr;
        check(bbk_hreads_stretch_view(b.hr, &r, &q), "bbk_hreads_stretch_view");
        check(bbk_kmerstats_push(ks, r, q), "bbk_kmerstats_push");
    });
    check(bbk_kmerstats_finish(ks), "bbk_kmerstats_finish");
    ph.device += now_s() - t0;

    t0 = now_s();
    const bool files_out = !p.prefix.empty();
    uint64_t changed_reads = 0;
    if (files_out) {
        std::vector<uint64_t> buf((size_t)n);  // one word per k-mer (k <= 32)
        check(bbk_kmerset_export(ctx, set, BBK_ORDER_SORTED, buf.data(), nullptr), "bbk_kmerset_export");
        write_u64(p.prefix + ".kmers", buf.data(), buf.size());
    }
    if (files_out && !p.subcluster) check(bbk_kmerstats_write(ctx, ks, (p.prefix + ".kmstat").c_str()), "bbk_kmerstats_write");
    if (hc) {
        if (files_out) check(bbk_hamclusters_write(ctx, hc, (p.prefix + ".hamming").c_str()), "bbk_hamclusters_write");
        info("Clustering done. Total clusters: %llu", (unsigned long long)bbk_hamclusters_count(hc));
    }
    if (p.subcluster) {
        bbk_subclusters *sc = nullptr;
        check(bbk_hamclusters_subcluster(ctx, set, hc, ks, &p.sp, &sc), "bbk_hamclusters_subcluster");
        if (p.expand) {
            bbk_expander *ex = expand_solid(ctx, set, sc, src, p.expand_max_iterations, p.expand_min_changed);
            if (p.correct) {
                CorrectedWriter w{files, groups, p.prefix, p.out_dir, ctx, nullptr, p.qvoffset, p.correct_stats, p.iteration, outlibs};
                changed_reads = correct_reads(set, ex, src, w, p.save_yaml);
            }
            bbk_expander_free(ex);
        }
        if (files_out) check(bbk_subclusters_write(ctx, sc, ks, p.prefix.c_str()), "bbk_subclusters_write");
        report_subclusters(ctx, sc);
        bbk_subclusters_free(sc);
    }
    if (hc) bbk_hamclusters_free(hc);
    {
        std::vector<uint32_t> cnt((size_t)n);
        check(bbk_kmerstats_export(ctx, ks, cnt.data(), nullptr, nullptr), "bbk_kmerstats_export");
        uint64_t singletons = 0;
        for (uint32_t c : cnt) singletons += c == 1;
        info("There are %llu kmers in total. Among them %llu (%g%%) are singletons.", (unsigned long long)n,
             (unsigned long long)singletons, n ? 100.0 * (double)singletons / (double)n : 0.0);
    }
    src.clear();
    bbk_kmerstats_free(ks);
    bbk_kmerset_free(set);
    ph.write += now_s() - t0;
    return changed_reads;
}

// mkdir -p of one level and the absolute name: the names in corrected.yaml are absolute (a reader resolves relative ones
// against the file)
inline std::string make_dir_absolute(const std::string &dir) {
    if (mkdir(dir.c_str(), 0755) != 0 && errno != EEXIST) fatal("cannot create %s", dir.c_str());
    char real[PATH_MAX];
    if (!realpath(dir.c_str(), real)) fatal("cannot resolve %s", dir.c_str());
    return real;
}

}  // namespace bbkhost
