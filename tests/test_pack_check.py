"""The device's ASCII -> stream step (kma_device.h: pack8 / store40, shared by the pack kernel
and the staged probe) against kma_pack_residues, on the host: kmers.anno_amd/host/pack_check.hip
is a stand-alone program built with -fsanitize=address,undefined that packs residues of every
length 0..130 at every misalignment, bytes without codes included, from and into buffers of
exact size, and compares the two streams. The test builds and runs it."""
import os
import subprocess

from conftest import PKG


def test_pack_routine_equals_host_packer_under_sanitizers(native_lib):
    subprocess.run(["make", "-s", "-C", PKG, "build/kma_pack_check"], check=True)
    exe = os.path.join(PKG, "build", "kma_pack_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pack_check ok: 4192 streams" in r.stdout
