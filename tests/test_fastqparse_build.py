"""CPU: the build of the device FASTQ parser -- the library exports its entry points, fastqparse.o holds exactly its four
kernels with no scratch and no spills, the binding has its classes, and the host programs have their new modes.  No GPU."""
import subprocess

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build, build_host

ENTRIES = ("bbk_fastq_input_from_host", "bbk_fastq_input_records", "bbk_fastq_input_verdict", "bbk_fastq_input_text_end",
           "bbk_fastq_input_records_within", "bbk_fastq_input_free", "bbk_hreads_from_fastq_input", "bbk_hreads_export_records",
           "bbk_hreads_bases", "bbk_hreads_name_bytes", "bbk_corrected_print_resident")
KERNELS = ("k_fq_count", "k_fq_lines", "k_fq_records", "k_fq_gather")


def test_library_exports_the_entries():
    build.build()
    L = B.load_library()
    missing = [e for e in ENTRIES if not hasattr(L, e)]
    assert not missing, missing
    assert "FastqInput" in B.__all__ and hasattr(B.Context, "fastq_input")
    assert all(hasattr(B.FastqInput, a) for a in ("records", "verdict", "text_end", "records_within", "hammer_reads"))
    assert hasattr(B.HammerReads, "records") and hasattr(B.Corrected, "print_resident")
    assert "fastqparse.hip" in build.SOURCES


def test_kernels_use_no_scratch():
    build.build()
    res = build.check_resources()
    if res is None:  # the llvm tools that read the metadata are not installed: the build warns, and so does this
        import warnings
        warnings.warn("llvm-objdump / llvm-readelf not found: the kernels' resources were not checked")
        return
    mine = [r for r in res if r[0] == "fastqparse.o"]
    for kname in KERNELS:
        rows = [r for r in mine if kname in r[1]]
        assert len(rows) == 1, (kname, [r[1] for r in mine])
        assert rows[0][2:] == (0, 0, 0), rows[0]  # scratch bytes, SGPR spills, VGPR spills
    assert len(mine) == len(KERNELS), [r[1] for r in mine]


def test_kmerdata_lists_the_option():
    exe = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--device-parse" in r.stdout and "--parse-chunk" in r.stdout


def test_fastx_dump_prints_records(tmp_path):
    exe = [e for e in build_host.build() if e.endswith("bbk-fastx-dump")][0]
    p = tmp_path / "two.fq"
    p.write_bytes(b"@a b\nacgtn\n+\nIIIII\n>f\nAC\nGT\n")
    r = subprocess.run([exe, "--records", str(p)], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"3 a b\n5 ACGTN\n5 IIIII\n1 f\n4 ACGT\n0 \n"
