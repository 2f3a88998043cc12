"""A check call that fails gives its device memory back (csrc/zv_checks.inc: every buffer of a
call belongs to its ChkDev, and a variant / mode combination is rejected before the first
allocation).  Each case is a call that returns an error code by design; the device's free memory
must not fall by the buffers the call would have made.  The reading is device-wide (other
processes share the card), so a case repeats its measure-call-measure sequence up to three times
and passes on the first clean reading; a leak strands L on every attempt."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _selftest(lib, M, N, K, variant, mode):
    d, r = ctypes.c_float(), ctypes.c_float()
    return lib.zv_gemm_selftest(M, N, K, variant, mode, ctypes.byref(d), ctypes.byref(r))


def _bench(lib, M, N, K, variant, iters, mode):
    ms = ctypes.c_float()
    return lib.zv_bench_gemm(M, N, K, variant, iters, mode, ctypes.byref(ms))


def _bv_post(lib, rows, C):
    """zv_bigvgan_check's conv_post with a channel count whose LDS window is past 64 KiB."""
    import numpy as np
    from zipvoice_amd.engine import ZvBigvganCheckArgs
    a = ZvBigvganCheckArgs()
    x, w, out = np.zeros((rows, C), np.float32), np.zeros((C, 7), np.float32), np.zeros(rows, np.float32)
    a.kind, a.split, a.B, a.Lmax, a.Ls, a.C, a.scale = 5, 1, 1, rows, rows, C, 1
    a.x, a.w, a.out = x.ctypes.data, w.ctypes.data, out.ctypes.data
    return lib.zv_bigvgan_check(ctypes.byref(a))


# (call, arguments, the reason zv_last_error names, bytes a leaking call strands: the selftest's two
# outputs and residual (3 fp32 M x N), the benchmark's fp32 C, conv_post's input stream)
CASES = [
    (_selftest, (4096, 4096, 64, 999, 0), "unknown variant", 3 * 4096 * 4096 * 4),
    (_selftest, (4096, 4096, 64, 70, 0), "residual-only variant", 3 * 4096 * 4096 * 4),
    (_bench, (8192, 8192, 64, 999, 1, 0), "unknown variant", 8192 * 8192 * 4),
    (_bv_post, (1 << 18, 256), "too wide for the LDS window", (1 << 18) * 256 * 4),
]


@pytest.mark.parametrize("call,args,reason,stranded", CASES,
                         ids=["selftest-unknown", "selftest-residual-only", "bench-unknown", "bigvgan-post-lds"])
def test_failed_check_frees_device_memory(call, args, reason, stranded):
    from zipvoice_amd import engine
    lib = engine.load_library()
    torch.cuda.init()
    falls = []
    for _ in range(3):
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        rc = call(lib, *args)
        err = lib.zv_last_error().decode()
        torch.cuda.synchronize()
        after = torch.cuda.mem_get_info()[0]
        assert rc != 0, (args, rc)
        assert reason in err, (args, err)
        falls.append(before - after)
        print(f"{call.__name__}{args}: rc {rc} '{err}', free memory fell by {falls[-1]} B "
              f"(a leak strands {stranded} B)")
        if falls[-1] < stranded // 2:
            return
    pytest.fail(f"free device memory fell by {falls} B over three failing calls; "
                f"each strands less than {stranded // 2} B if the call frees its buffers")
