"""CPU: the build of the prepared read batch -- the library exports its entry points, its kernels are in the resource
report with no scratch and no spills, and the host programs link against it.  No GPU."""
import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build, build_host

ENTRIES = ("bbk_hreads_from_host", "bbk_hreads_size", "bbk_hreads_kmer_stretches", "bbk_hreads_corrector_stretches",
           "bbk_hreads_candidates", "bbk_hreads_export", "bbk_hreads_stretch_view", "bbk_hreads_candidate_view",
           "bbk_corrector_correct_prepared", "bbk_hreads_free")
KERNELS = ("k_hr_prepareILb0E", "k_hr_prepareILb1E", "k_hr_ranges", "k_hr_pack", "k_hr_copy")


def test_library_exports_the_entries():
    build.build()
    L = B.load_library()
    missing = [e for e in ENTRIES if not hasattr(L, e)]
    assert not missing, missing
    assert "HammerReads" in B.__all__ and hasattr(B.Corrector, "correct_prepared") and hasattr(B.Context, "hammer_reads")
    assert "NO_TRIM" in B.__all__ and B.NO_TRIM == -2 ** 31  # BBK_NO_TRIM of include/bbk.h: INT_MIN
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbk.h")).read()
    assert "#define BBK_NO_TRIM (-2147483647 - 1)" in header


def test_kernels_use_no_scratch():
    build.build()
    res = build.check_resources()
    if res is None:  # the llvm tools that read the metadata are not installed: the build warns, and so does this
        import warnings
        warnings.warn("llvm-objdump / llvm-readelf not found: the kernels' resources were not checked")
        return
    mine = [r for r in res if r[0] == "hreads.o"]
    for kname in KERNELS:
        rows = [r for r in mine if kname in r[1]]
        assert len(rows) == 1, (kname, [r[1] for r in mine])
        assert rows[0][2:] == (0, 0, 0), rows[0]  # scratch bytes, SGPR spills, VGPR spills
    assert len(mine) == len(KERNELS), [r[1] for r in mine]


def test_host_programs_link():
    exes = build_host.build()
    assert any(e.endswith("spades-kmerdata") for e in exes) and any(e.endswith("bbk-hammer-reads-dump") for e in exes)
    import subprocess
    exe = [e for e in exes if e.endswith("spades-kmerdata")][0]
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--resident-bytes" in r.stdout
