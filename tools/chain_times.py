"""Per-launch time of the launches whose loads were re-placed (fused FFN block; k-split / wave-private GEMM configurations with and
without a residual), by the method of profiles/r8_ab_ln_reduce_stem_b1_q1000.txt: HIP events around a captured dependent chain of 64
launches, operands rotating through 8 buffers so that every launch finds them L2-cold, as in the forward.  Run it once per library
build (parent, branch) in the same visit.  GPU box:  python tools/chain_times.py [label]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cotr_amd import _lib
lib = _lib.load_library()
dev = torch.device('cuda:0')
P = lambda t: None if t is None else t.data_ptr()
CHAIN, NBUF = 64, 8
label = sys.argv[1] if len(sys.argv) > 1 else ''


def chain_us(launch, per_step=1):
    """launch(i, stream pointer) enqueues step i of the chain -> best-of-5 microseconds per launch"""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sp = s.cuda_stream
        for i in range(3):
            assert launch(i, sp) == 0
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(CHAIN):
                launch(i, sp)
        g.replay(); s.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e9
        for _ in range(5):
            e0.record(s)
            for _ in range(4):
                g.replay()
            e1.record(s); s.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1000 / (4 * CHAIN * per_step))
    return best


for M in (1000, 512):
    w1 = [torch.randn(1024, 256, device=dev) / 16 for _ in range(NBUF)]
    w2 = [torch.randn(256, 1024, device=dev) / 32 for _ in range(NBUF)]
    b1, b2 = torch.randn(1024, device=dev) * 0.1, torch.randn(256, device=dev) * 0.1
    lw, lb = torch.ones(256, device=dev), torch.zeros(256, device=dev)
    ys = [torch.randn(M, 256, device=dev) for _ in range(2)]
    nch = lib.cotr_op_ffn_chunks(M)
    scratch = [torch.empty(nch * M * 256, device=dev) for _ in range(NBUF)]
    run = lambda i, sp: lib.cotr_op_ffn_block(P(ys[(i + 1) & 1]), P(w1[i % NBUF]), P(b1), P(w2[i % NBUF]), P(b2), P(lw), P(lb),
                                              P(scratch[i % NBUF]), P(ys[i & 1]), M, sp)
    t = [chain_us(run) for _ in range(2)]
    print(f'{label} ffn_block chain (ffn_fused x{nch} + ln_reduce), {M} rows, weights L2-cold: ' + '  '.join(f'{v:6.2f} us' for v in t), flush=True)

for cfg, M, N, K in [(36, 2048, 512, 128), (36, 512, 1024, 256), (39, 512, 256, 1024), (25, 512, 768, 256)]:
    xs = [torch.randn(M, K, device=dev) for _ in range(NBUF)]
    ws = [torch.randn(N, K, device=dev) / K ** 0.5 for _ in range(NBUF)]
    bias = torch.randn(N, device=dev)
    rs = [torch.randn(M, N, device=dev) for _ in range(NBUF)]
    ys = [torch.empty(M, N, device=dev) for _ in range(2)]
    for with_res in (True, False):
        run = lambda i, sp: lib.cotr_op_linear_cfg(P(xs[i % NBUF]), P(ws[i % NBUF]), P(bias), P(rs[i % NBUF]) if with_res else None, 1,
                                                   P(ys[i & 1]), M, N, K, cfg, sp)
        t = [chain_us(run) for _ in range(2)]
        print(f'{label} linear chain cfg {cfg} {M}x{N}x{K} bias relu{" residual" if with_res else ""}, operands L2-cold: ' +
              '  '.join(f'{v:6.2f} us' for v in t), flush=True)
