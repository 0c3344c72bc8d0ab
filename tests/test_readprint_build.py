"""CPU: the build of the device FASTQ printer -- the library exports its entry points, readprint.o holds exactly its three
kernels with no scratch and no spills, and spades-kmerdata lists the options that reach them.  No GPU."""
import subprocess

import spades_for_blackbird_amd as B
from spades_for_blackbird_amd import build, build_host

ENTRIES = ("bbk_corrector_correct_resident", "bbk_corrected_size", "bbk_corrected_export", "bbk_corrected_free",
           "bbk_corrected_print", "bbk_fastq_text_streams", "bbk_fastq_text_size", "bbk_fastq_text_export",
           "bbk_fastq_text_write", "bbk_fastq_text_free")
KERNELS = ("k_rp_outcome", "k_rp_size", "k_rp_write")


def test_library_exports_the_entries():
    build.build()
    L = B.load_library()
    missing = [e for e in ENTRIES if not hasattr(L, e)]
    assert not missing, missing
    assert "Corrected" in B.__all__ and "FastqText" in B.__all__
    assert hasattr(B.Corrector, "correct_resident") and hasattr(B.Corrected, "print") and hasattr(B.Corrected, "export")
    assert all(hasattr(B.FastqText, a) for a in ("sizes", "stream", "write"))
    assert "readprint.hip" in build.SOURCES


def test_kernels_use_no_scratch():
    build.build()
    res = build.check_resources()
    if res is None:  # the llvm tools that read the metadata are not installed: the build warns, and so does this
        import warnings
        warnings.warn("llvm-objdump / llvm-readelf not found: the kernels' resources were not checked")
        return
    mine = [r for r in res if r[0] == "readprint.o"]
    for kname in KERNELS:
        rows = [r for r in mine if kname in r[1]]
        assert len(rows) == 1, (kname, [r[1] for r in mine])
        assert rows[0][2:] == (0, 0, 0), rows[0]  # scratch bytes, SGPR spills, VGPR spills
    assert len(mine) == len(KERNELS), [r[1] for r in mine]


def test_kmerdata_lists_the_options():
    exe = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--paired", "--correct-stats", "--output-dir"):
        assert opt in r.stdout, opt


def test_paired_input_is_checked_before_the_device(tmp_path):
    """what --paired refuses is refused from the file lists alone: an odd number of files, an interlaced library, a
    library whose left and right lists differ in length"""
    exe = [e for e in build_host.build() if e.endswith("spades-kmerdata")][0]

    def run(args):
        return subprocess.run([exe, "-o", str(tmp_path / "o"), "--correct", "--paired"] + args, capture_output=True, text=True,
                              timeout=60)

    r = run(["a.fq", "b.fq", "c.fq"])
    assert r.returncode != 0 and "3 input files: a pair is a left and a right file" in r.stderr
    y = str(tmp_path / "d.yaml")
    with open(y, "w") as f:
        f.write('- orientation: "fr"\n  type: "paired-end"\n  interlaced reads:\n    - "i.fq"\n')
    r = run(["-d", y])
    assert r.returncode != 0 and "interlaced" in r.stderr and "i.fq" in r.stderr
    with open(y, "w") as f:
        f.write('- type: "paired-end"\n  left reads:\n    - "l1.fq"\n    - "l2.fq"\n  right reads:\n    - "r1.fq"\n')
    r = run(["-d", y])
    assert r.returncode != 0 and "2 left and 1 right read files" in r.stderr
