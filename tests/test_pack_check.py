"""The device's ASCII -> stream step (kma_device.h: pack8 / store40, shared by the pack kernel
and the staged probe) against the host packer, on the host: kmers.anno_amd/host/pack_check.hip
is a stand-alone program built with -fsanitize=address,undefined, csrc/kma_pack.cpp compiled into
it with the same flags (the AVX2 packer itself is instrumented), that packs residues of every
length 0..130 at every misalignment and of lengths around the 512-residue non-temporal blocks
into 64-byte aligned and misaligned outputs, with the standard alphabet and with one and four
extra table symbols, bytes without codes and all 256 byte values included, from and into buffers
of exact size, and compares the streams. The test builds and runs it."""
import os
import subprocess

from conftest import PKG

# per LUT: 5 patterns x (131 lengths x 8 misalignments + 5 long lengths x 3 output offsets x 2
# input misalignments); the standard LUT twice (kma::pack_residues_host and kma_pack_residues)
STREAMS = 4 * 5 * (131 * 8 + 5 * 3 * 2)


def test_pack_routine_equals_host_packer_under_sanitizers(native_lib):
    subprocess.run(["make", "-s", "-C", PKG, "build/kma_pack_check"], check=True)
    exe = os.path.join(PKG, "build", "kma_pack_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert STREAMS == 21560 and f"pack_check ok: {STREAMS} streams" in r.stdout
