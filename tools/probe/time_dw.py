"""A/B of gf_linear_dw / gf_linear_dw2 between two builds of the library: python tools/probe/time_dw.py libA.so libB.so
Per shape: best-of-4 microseconds per call, A B A B, then max|dW_A - dW_B| and max|db_A - db_B| on the same inputs.
The train step's five bf16 shapes at M = 131072 (all on the LDS-DMA kernel), then one small shape for each other way into
csrc/linear_dw.hip: fp32, bf16 off the 128-multiples, two sources."""
import ctypes, sys, torch
P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
g = torch.Generator(device="cuda").manual_seed(0)
def timeit(fn, iters=20):
    for _ in range(5): fn()
    best = 1e9
    for _ in range(4):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters): fn()
        b.record(); torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best
libs = []
for path in sys.argv[1:]:
    lib = ctypes.CDLL(path)
    lib.gf_linear_dw_ws_bytes.restype = L
    lib.gf_linear_dw_ws_bytes.argtypes = [I, I, I]
    lib.gf_linear_dw.argtypes = [P, P, P, P, P, I, I, I, I, P]
    lib.gf_linear_dw2.argtypes = [P, P, P, I, P, P, P, I, I, I, I, P]
    libs.append(lib)
# (M, Nout, K, K1 of a two-source call or 0, dtype)
SHAPES = [(131072, nout, k, 0, torch.bfloat16) for nout, k in ((768, 256), (256, 256), (512, 256), (256, 512), (512, 512))]
SHAPES += [(4100, 136, 72, 0, torch.float32), (4100, 136, 72, 0, torch.bfloat16), (4100, 256, 384, 128, torch.bfloat16)]
for M, nout, k, k1, dtype in SHAPES:
    dy = torch.randn(M, nout, device="cuda", generator=g).to(dtype)
    x = torch.randn(M, k, device="cuda", generator=g).to(dtype)
    xa, xb = (x[:, :k1].contiguous(), x[:, k1:].contiguous()) if k1 else (x, None)
    code = 0 if dtype == torch.float32 else 1
    st = torch.cuda.current_stream().cuda_stream
    row, outs = [], []
    for lib in libs + libs:
        ws = torch.empty(int(lib.gf_linear_dw_ws_bytes(M, nout, k)), dtype=torch.uint8, device="cuda")
        dw, db = torch.empty(nout, k, device="cuda"), torch.empty(nout, device="cuda")
        if k1:
            fn = lambda: lib.gf_linear_dw2(dy.data_ptr(), xa.data_ptr(), xb.data_ptr(), k1, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), M, nout, k, code, st)
        else:
            fn = lambda: lib.gf_linear_dw(dy.data_ptr(), xa.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), M, nout, k, code, st)
        assert fn() == 0
        row.append(f"{timeit(fn)*1e3:7.1f}")
        outs.append((dw, db))
    diff = ""
    if len(libs) == 2:
        diff = (f"  max|dW_A-dW_B| = {float((outs[0][0] - outs[1][0]).abs().max()):g}"
                f"  max|db_A-db_B| = {float((outs[0][1] - outs[1][1]).abs().max()):g}")
    print(f"M={M} {nout}x{k}{f' ({k1}+{k - k1})' if k1 else ''} {str(dtype)[6:]}: " + " ".join(row) + diff, flush=True)
