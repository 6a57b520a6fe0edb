"""kma_last_error is per thread (include/kmeranno.h: "the message of the last failure on the
calling thread"): a JNI host calls from several threads and turns a failed call's message into
its exception, so one thread's failure must not show up in, or overwrite, another's. The failing
calls here touch no device (kma_option_set with a value out of range, kma_table_wrap_device with
a layout code that does not exist), so the test runs without a GPU."""
import ctypes as C
import threading

E_INVALID = -1
OPT_BLOCK_PROTEINS, OPT_DEFER = 2, 3


def test_last_error_is_thread_local(native_lib):
    lib = native_lib
    barrier = threading.Barrier(4)
    seen, errors = {}, []

    def bad_option(option, value):
        return lambda: lib.kma_option_set(option, value)

    def bad_layout():
        out = C.c_void_p()
        buf = (C.c_uint64 * 64)()
        rc = lib.kma_table_wrap_device(C.addressof(buf), 8, 8, 5, 0, C.byref(out))
        assert out.value is None
        return rc

    def run(name, call):
        try:
            rc = call() if call else 0
            barrier.wait(timeout=60)            # every failing call has been made
            first = lib.kma_last_error().decode()
            barrier.wait(timeout=60)            # every thread has read once
            seen[name] = (rc, first, lib.kma_last_error().decode())
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append((name, e))

    calls = {"block": bad_option(OPT_BLOCK_PROTEINS, 99), "defer": bad_option(OPT_DEFER, 1000),
             "layout": bad_layout, "quiet": None}
    threads = [threading.Thread(target=run, args=kv) for kv in calls.items()]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors and not any(t.is_alive() for t in threads)
    for name in ("block", "defer", "layout"):
        assert seen[name][0] == E_INVALID, name
        assert seen[name][1] and seen[name][1] == seen[name][2], name
    assert seen["block"][1] == f"option {OPT_BLOCK_PROTEINS}: value 99 out of range"
    assert seen["defer"][1] == f"option {OPT_DEFER}: value 1000 out of range"
    assert seen["layout"][1].startswith("layout 5 is not 0")
    assert seen["quiet"] == (0, "", "")  # a thread that made no failing call sees neither
    # the options the failed calls named are unchanged
    v = C.c_int64(-5)
    assert lib.kma_option_get(OPT_BLOCK_PROTEINS, C.byref(v)) == 0 and v.value == 0
    assert lib.kma_option_get(OPT_DEFER, C.byref(v)) == 0 and v.value == -1
