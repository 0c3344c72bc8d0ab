"""CPU: the host side of spades-hammer -- determine_offset through bbk-fastx-dump --offset against a
restatement, what the driver refuses before it touches the device, and the build of the minimum-count filter: the entry
point, the binding, kmerfilter.o's kernels and the option of spades-kmerdata.  No GPU."""
import inspect
import os
import subprocess

import pytest

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build, build_host, engine
from tests import fastq_restated as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kmerfilter.o's kernels: its instantiations of the ordered selection (select.h), as kernel<first template argument: the
# predicate> -- the count of the filter and the count-only selection of the dropped self-complementary records -- and the
# filter's own write kernel
KERNELS = ("k_select_count<McKept>", "k_select_count<McDroppedSelfRc>", "k_mc_write")


def is_kernel(kname, mangled):
    """the mangled name is an instantiation of `kname` (kernel<Predicate> or kernel) for some key width"""
    kernel, _, pred = kname.rstrip(">").partition("<")
    head = "%d%sI" % (len(kernel), kernel)
    return (head + "NS_%d%sILi" % (len(pred), pred) if pred else head + "Li") in mangled


@pytest.fixture(scope="module")
def bins():
    build.build()
    return {os.path.basename(p): p for p in build_host.build()}


def determine_offset(data):
    """determine_offset (common/io/reads/ireadstream.hpp:154-170) over the text of a file"""
    for _, _, qual in FR.records(data)[:10000]:
        for c in qual:
            q = c - 256 if c > 127 else c  # the bytes are signed chars there
            if q < ord(";"):
                return "33"
            if q > ord("K"):
                return "64"
    return "failed"


def neutral(n, first=0):
    """n records whose quality bytes decide nothing: all within [';', 'K']"""
    return b"".join(FR.fq("r%d" % (first + i), "ACGTACGTAC", qual=b";<=>?@ABJK") for i in range(n))


OFFSET_CASES = {
    "phred33": (FR.fq("a", "ACGT", qual="II#I") + FR.fq("b", "ACGT", qual="hhhh"), "33"),
    "phred64": (FR.fq("a", "ACGT", qual="KKhK") + FR.fq("b", "ACGT", qual="####"), "64"),
    "deciding_byte_in_record_10000": (neutral(9999) + FR.fq("d", "ACGT", qual="KKKL") + neutral(5, 10000), "64"),
    "deciding_byte_in_record_10001": (neutral(10000) + FR.fq("d", "ACGT", qual="!!!!") + neutral(5, 10001), "failed"),
    "multi_line_record": (b"@m\nACGT\nACGT\n+m\n@@@@\n@@:@\n" + neutral(3), "33"),
    "short_file_undecided": (neutral(7), "failed"),
    "empty_file": (b"", "failed"),
    "high_byte_is_negative": (FR.fq("a", "ACGT", qual=b"@@\xc8@"), "33"),
    "fasta_then_fastq": (b">f\nACGT\n" + FR.fq("a", "ACGT", qual="@@@Z"), "64"),
}


@pytest.mark.parametrize("case", sorted(OFFSET_CASES))
def test_determine_offset(bins, tmp_path, case):
    data, expected = OFFSET_CASES[case]
    assert determine_offset(data) == expected  # the restatement says what the case is meant to show
    p = tmp_path / (case + ".fq")
    p.write_bytes(data)
    r = subprocess.run([bins["bbk-fastx-dump"], "--offset", str(p)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == expected + "\n", (r.stdout, r.stderr)


def test_determine_offset_of_a_missing_file(bins):
    r = subprocess.run([bins["bbk-fastx-dump"], "--offset", "/nonexistent/x.fq"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "cannot open" in r.stderr


def shipped_config(**subst):
    """the shipped config.info with values substituted as the pipeline's stage script does"""
    out = []
    for line in open(os.path.join(ROOT, "tests", "golden", "hammer_config.info")).read().split("\n"):
        key = line.split()[0] if line.split() else ""
        out.append("%s %s" % (key, subst.pop(key)) if key in subst else line)
    assert not subst, subst
    return "\n".join(out)


def test_refusals_come_before_the_device(bins, tmp_path):
    """no row reaches bbk_ctx_create (there is no GPU here): the message is the driver's own"""
    exe = bins["spades-hammer"]

    def run(config_text=None, path=None, cwd=None):
        if config_text is not None:
            path = str(tmp_path / "config.info")
            with open(path, "w") as f:
                f.write(config_text)
        r = subprocess.run([exe] + ([path] if path else []), capture_output=True, text=True, timeout=60, cwd=cwd or str(tmp_path))
        assert "bbk_ctx_create" not in r.stderr
        return r

    r = run(path="/nonexistent/config.info")
    assert r.returncode == 255 and "cannot open config file /nonexistent/config.info" in r.stderr
    empty = tmp_path / "empty"
    empty.mkdir()
    r = run(cwd=str(empty))  # no argument: config.info of the current directory
    assert r.returncode == 255 and "cannot open config file config.info" in r.stderr
    r = run(shipped_config(general_tau="2"))
    assert r.returncode == 255 and "general_tau 2" in r.stderr
    for key, value in (("bayes_use_hamming_dist", "1"), ("bayes_hammer_mode", "1"), ("bayes_initial_refine", "0"), ("count_do", "0"),
                       ("hamming_do", "0"), ("bayes_do", "0"), ("expand_do", "0"), ("correct_do", "0"),
                       ("expand_write_each_iteration", "1")):
        r = run(shipped_config(**{key: value}))
        assert r.returncode == 255 and "%s %s" % (key, value) in r.stderr, (key, r.stderr)
    r = run(shipped_config().replace("correct_stats", "; correct_stats"))
    assert r.returncode == 255 and "(correct_stats)" in r.stderr
    r = run(shipped_config(dataset="/nonexistent/dataset.yaml"))
    assert r.returncode == 255 and "cannot open dataset file /nonexistent/dataset.yaml" in r.stderr
    y = tmp_path / "d.yaml"
    y.write_text('- orientation: "fr"\n  type: "paired-end"\n  interlaced reads:\n    - "i.fq"\n')
    r = run(shipped_config(dataset=str(y)))
    assert r.returncode == 255 and "interlaced" in r.stderr and "i.fq" in r.stderr
    # an offset that cannot be determined: the reference's words and exit(-1), no directory made
    fq = tmp_path / "undecided.fq"
    fq.write_bytes(neutral(4))
    y.write_text('- type: "single"\n  single reads:\n    - "%s"\n' % fq)
    r = run(shipped_config(dataset=str(y), output_dir=str(tmp_path / "out"), input_working_dir=str(tmp_path / "out" / "tmp")))
    assert r.returncode == 255 and "Failed to determine offset! Specify it manually and restart, please!" in r.stderr
    assert "Trying to determine PHRED offset" in r.stdout and not (tmp_path / "out").exists()


def test_library_exports_the_entry():
    build.build()
    L = B.load_library()
    assert hasattr(L, "bbk_count_finish_min_count")
    assert "bbk_count_finish_min_count" in engine.SYMBOLS
    assert "min_count" in inspect.signature(engine.Counter.finish).parameters
    assert inspect.signature(engine.Counter.finish).parameters["min_count"].default is None
    assert "kmerfilter.hip" in build.SOURCES
    assert "spades-hammer" in build_host.PROGRAMS and {"hammer_run.hpp", "hammer_config.hpp"} <= set(build_host.HEADERS)


def test_kernels_use_no_scratch():
    build.build()
    res = build.check_resources()
    if res is None:  # the llvm tools that read the metadata are not installed: the build warns, and so does this
        import warnings
        warnings.warn("llvm-objdump / llvm-readelf not found: the kernels' resources were not checked")
        return
    mine = [r for r in res if r[0] == "kmerfilter.o"]
    for kname in KERNELS:  # one instantiation per key width
        rows = [r for r in mine if is_kernel(kname, r[1])]
        assert len(rows) == 4, (kname, [r[1] for r in mine])
        assert all(r[2:] == (0, 0, 0) for r in rows), rows  # scratch bytes, SGPR spills, VGPR spills
    assert len(mine) == 4 * len(KERNELS), [r[1] for r in mine]


def test_kmerdata_lists_the_option(bins):
    r = subprocess.run([bins["spades-kmerdata"], "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--filter-singletons" in r.stdout
