"""CPU-only: the C-ABI library loads and exports every symbol include/bbk.h declares, the host
programs honour the reference's argv contracts, and the host FASTA/FASTQ reader follows kseq."""
import gzip
import os
import re
import subprocess

import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build, build_host, engine
from tests.helpers import read_fastq_gz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bins():
    build.build()
    return {os.path.basename(p): p for p in build_host.build()}


def test_library_exports_every_declared_symbol():
    build.build()
    L = B.load_library()
    hdr = open(os.path.join(ROOT, "include", "bbk.h")).read()
    declared = set(re.findall(r"\b(bbk_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations found"
    for sym in sorted(declared):
        assert hasattr(L, sym), "libbbk.so does not export %s" % sym
    assert declared == set(engine.SYMBOLS)
    assert L.bbk_words(21) == 1 and L.bbk_words(33) == 2 and L.bbk_words(127) == 4
    assert b"gfx950" in L.bbk_version()


def test_no_cpu_fallback():
    """Without a GPU the product path must fail loudly (never route through the oracle)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(B.BBKError):
        B.Context(0)
    src = ""
    for dp, _, fs in os.walk(os.path.join(ROOT, "spades_for_blackbird_amd")):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".hpp", ".cpp")):
                src += open(os.path.join(dp, f), errors="replace").read()
    assert "import oracle" not in src and "from oracle" not in src and "liboracle" not in src


Y = "/nonexistent/d.yaml"
USAGE = (1, "stdout", "SYNOPSIS")  # the usage text and exit(1)
REQ = ["-k", "21", "-n", "2", "-s", "1", "-o", "p", "-f", "/nonexistent"]  # kmer_multiplicity_counter's required options
ABU = ["-k", "21", "-n", "2", "-c", "c", "-m", "m", "-o", "o"]             # contig_abundance_counter's

# (tool, argv, exit code, stream, words that must appear there); every row ends before the first HIP call
ARGV_ROWS = [
    ("spades-kmercount", [], 255, "stderr", "No input files were specified"),
    ("spades-kmercount", ["-h"], 0, "stdout", ("--kmer", "final_kmers")),
    ("spades-kmercount", ["--bogus", "x.fa"], *USAGE),
    ("spades-kmercount", ["-k"], *USAGE),
    ("spades-kmercount", ["-k", "x", "a.fa"], *USAGE),
    ("spades-kmercount", ["-k", "notanumber", "x.fa"], *USAGE),
    ("spades-kmercount", ["-k", "128", "a.fa"], 255, "stderr", "out of range"),
    ("spades-kmercount", ["-k", "0", "a.fa"], 255, "stderr", "out of range"),
    ("spades-kmercount", ["--devices", "a,b", "a.fa"], 255, "stderr", "comma-separated"),
    ("spades-kmercount", ["--exchange", "x", "a.fa"], 255, "stderr", "rccl or copy"),
    ("spades-kmercount", ["-d", Y], 255, "stderr", "cannot open dataset"),
]
for _tool in ("spades-hamcluster", "spades-kmerdata"):
    ARGV_ROWS += [
        (_tool, [], 255, "stderr", "No input files were specified"),
        (_tool, ["-h"], 0, "stdout", "SYNOPSIS"),
        (_tool, ["a.fq"], *USAGE),
        (_tool, ["-k", "33", "-o", "p", "a.fq"], 255, "stderr", "out of range [1, 32]"),
        (_tool, ["-o", "p", "-d", Y], 255, "stderr", "cannot open dataset"),
    ]
ARGV_ROWS += [
    ("spades-hamcluster", ["--chunk", "-o", "p", "a.fq"], *USAGE),
    ("spades-kmerdata", ["--singleton-threshold", "abc", "-o", "p", "a.fq"], *USAGE),
    ("spades-kmerdata", ["--singleton-threshold"], *USAGE),
    ("spades-kmerdata", ["--qvoffset", "256", "-o", "p", "a.fq"], 255, "stderr", "out of range"),
    ("spades-kmerdata", ["--trim-quality", "94", "-o", "p", "a.fq"], 255, "stderr", "out of range"),
    ("spades-gbuilder", [], 1, "stdout", ("SYNOPSIS", "--gfa")),
    ("spades-gbuilder", ["a", "b", "-k", "22"], 255, "stderr", "must be odd"),
    ("spades-gbuilder", ["in.fa", "out.gfa", "-k", "22", "--gfa"], 255, "stderr", "k-mer size must be odd"),
    ("spades-gbuilder", ["a", "b", "-k", "129"], 255, "stderr", "too high"),
    ("spades-gbuilder", ["a", "b", "-k", "0"], 255, "stderr", "too low"),
    ("spades-gbuilder", ["a", "b", "--gfa", "--fastg"], *USAGE),
    ("spades-gbuilder", ["a", "b", "c"], *USAGE),
    ("spades-gbuilder", ["a", "b", "--early-tip-clip"], *USAGE),
    ("spades-gbuilder", ["a", "b", "--early-tip-clip", "4294967296"], *USAGE),
    ("spades-gbuilder", ["/nonexistent/a", "b", "--gfa", "-tmp-dir", "t"], 255, "stderr", "does not exist"),
    ("spades-gbuilder", ["/nonexistent/in.fa", "out.gfa", "--gfa"], 255, "stderr", "does not exist"),
    ("spades-gbuilder", ["/nonexistent/a.yaml", "b"], 255, "stderr", "cannot open dataset"),
]
for _tool in ("spades-kmer-estimating", "spades-read-filter"):
    ARGV_ROWS += [
        (_tool, [], *USAGE),
        (_tool, ["-h"], 0, "stdout", "SYNOPSIS"),
        (_tool, ["-d", Y, "extra"], *USAGE),
        (_tool, ["-d", Y], 255, "stderr", "cannot open dataset"),
    ]
ARGV_ROWS += [
    ("spades-kmer-estimating", ["-k", "0", "-d", Y], 255, "stderr", "out of range"),
    ("spades-kmer-estimating", ["-t", "x", "-d", Y], *USAGE),
    ("spades-read-filter", ["-k", "128", "-d", Y], 255, "stderr", "out of range"),
]
for _tool, _tmp in (("unitig-coverage", "--tmpdir"), ("spades-gmapper", "--tmp-dir")):
    ARGV_ROWS += [
        (_tool, [], *USAGE),
        (_tool, ["a", "b"], *USAGE),
        (_tool, [Y, "g.gfa", "o", "-k", "22"], 255, "stderr", "must be odd"),
        (_tool, [Y, "g.gfa", "o", "-k", "1000"], *USAGE),
        (_tool, [Y, "g.gfa", "o", "-k", "999"], 255, "stderr", "too high"),
        (_tool, [Y, "g.gfa", "o", "-b", "0"], *USAGE),
        (_tool, [Y, "g.txt", "o"], 255, "stderr", "only a GFA graph"),
        (_tool, [Y, "g.gfa", "o", _tmp, "t"], 255, "stderr", "cannot open dataset"),
    ]
ARGV_ROWS += [
    ("kmer_multiplicity_counter", [], 1, "stdout", "Usage"),
    ("kmer_multiplicity_counter", [a for a in REQ if a not in ("-s", "1")], 1, "stdout", "Usage"),
    ("kmer_multiplicity_counter", ["-k", "200"] + REQ[2:], 255, "stderr", "out of range"),
    ("kmer_multiplicity_counter", REQ[:2] + ["-n", "0"] + REQ[4:], 255, "stderr", "sample count"),
    ("kmer_multiplicity_counter", REQ + ["-b", "0"], 1, "stdout", "Usage"),
    ("kmer_multiplicity_counter", REQ + ["--cs", "70000"], 255, "stderr", "16-bit"),
    ("kmer_multiplicity_counter", REQ + ["--ci", "0"], 255, "stderr", "at least 1"),
    ("kmer_multiplicity_counter", REQ, 255, "stderr", "sample 1: none of"),
    ("kmer_multiplicity_counter", REQ + ["word"], 1, "stdout", "Usage"),
    ("contig_abundance_counter", [], 1, "stdout", "Usage"),
    ("contig_abundance_counter", ["-k", "200"] + ABU[2:], 255, "stderr", "out of range"),
    ("contig_abundance_counter", ABU[:2] + ["-n", "0"] + ABU[4:], 255, "stderr", "sample count"),
    ("contig_abundance_counter", ABU + ["-b", "0"], 1, "stdout", "Usage"),
    ("contig_abundance_counter", ABU[:-2], 1, "stdout", "Usage"),
    # a value that does not fit its destination, or carries a sign, is a usage error (it used to be truncated / wrapped)
    ("spades-kmercount", ["-k", "4294967317", "-d", Y], *USAGE),
    ("spades-hamcluster", ["-k", "4294967317", "-o", "p", "-d", Y], *USAGE),
    ("spades-kmercount", ["-k", "-5", "a.fa"], *USAGE),
]


def test_argv_contracts(bins, tmp_path):
    """The argv contract of the ten GPU tools: exit code, and the stream a given word appears on."""
    for tool, argv, code, stream, words in ARGV_ROWS:
        r = subprocess.run([bins[tool]] + argv, capture_output=True, text=True, cwd=str(tmp_path))
        row = (tool, argv, r.returncode, r.stdout[-300:], r.stderr[-300:])
        assert r.returncode == code, row
        for w in (words,) if isinstance(words, str) else words:
            assert w in getattr(r, stream), row


def _dump(bins, path):
    r = subprocess.run([bins["bbk-fastx-dump"], path], capture_output=True, text=True)
    assert r.returncode == 0
    return r.stdout.split("\n")[:-1]


def test_fastx_reader(bins, golden_dir, tmp_path):
    p = os.path.join(golden_dir, "ecoli_1K_1.fq.gz")
    assert _dump(bins, p) == read_fastq_gz(p)
    fa = tmp_path / "a.fa"
    fa.write_text(">r1 some comment\nACGT\nacgtnn\n\nGG\n>r2\nTTTT\n>empty\n>r3\nAC\n")
    assert _dump(bins, str(fa)) == ["ACGTACGTNNGG", "TTTT", "", "AC"]
    fq = tmp_path / "b.fq"
    fq.write_text("@a\nACGT\n+\nIIII\n@b\nGGCC\nTT\n+b\nIIII\nII\n@c\nACGTAC\n+\nIII\n@d\nAAAA\n+\nIIII\n")
    # record c has a truncated quality string: the reference's parser stops there (kseq -2 -> eof)
    assert _dump(bins, str(fq)) == ["ACGT", "GGCCTT"]
    gz = tmp_path / "c.fa.gz"
    with gzip.open(gz, "wt") as f:
        f.write(">x\nACGTNACGT\n")
    assert _dump(bins, str(gz)) == ["ACGTNACGT"]


def test_dataset_yaml(bins, golden_dir, tmp_path):
    """YAML forms written by spades.py / the reference's configs (assembler/configs/debruijn/toy.yaml)."""
    y = tmp_path / "toy.yaml"
    y.write_text("- left reads: [%s/ecoli_1K_1.fq.gz]\n  orientation: fr\n  right reads: [%s/ecoli_1K_2.fq.gz]\n"
                 "  type: paired-end\n" % (golden_dir, golden_dir))
    exe = bins["spades-kmercount"]
    r = subprocess.run([exe, "-d", str(y), "-w", str(tmp_path)], capture_output=True, text=True)
    # parsing succeeded iff we get as far as opening the device (no GPU here) or finishing (GPU box)
    assert "ecoli_1K_1.fq.gz" in r.stdout or "bbk_ctx_create" in r.stderr


def test_no_kernel_uses_scratch():
    """Build hygiene (scratch computes correctly on this pool; it costs occupancy): "no scratch, no VGPR
    spills" is enforced on the code-object metadata of every kernel of the built library."""
    from spades_for_blackbird_amd import build as b
    b.build()
    res = b.check_resources()
    if res is None:
        pytest.skip("llvm-objdump / llvm-readelf not installed")
    assert len(res) > 150  # all instantiations of all eight translation units are seen
    assert all(r[2] == 0 and r[4] == 0 for r in res)


def test_final_kmers_merge_of_shards_fuzz(tmp_path):
    """host/multi.hpp: write_final_kmers_merged (the writer of `spades-kmercount --devices`) against a plain sort, for
    1..8 shards, 1..4-word records, empty shards / buckets; host-only, AddressSanitizer + UBSan."""
    from spades_for_blackbird_amd import build as b
    b.build()
    exe = str(tmp_path / "merge_fuzz")
    lib = os.path.join(ROOT, "spades_for_blackbird_amd")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "merge_fuzz.cpp"), "-L" + lib, "-lbbk", "-lz", "-Wl,-rpath," + lib])
    for seed in (1, 2, 3):
        r = subprocess.run([exe, str(seed), str(tmp_path / "merged.bin")], capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0 and "MERGE-FUZZ-OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
