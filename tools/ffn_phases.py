"""Phase timestamps of the fused FFN kernel (cotr_debug_ffn_times) at the one-pair row counts.  GPU box.

The 8 slots per workgroup, as ffn_fused_pipe_kernel (csrc/ffn_pipe.hip, the form both row counts run) writes them; slots 0-3 and 5 are taken by
wavefront 0 (phase-1 role), slots 4, 6 and 7 by wavefront 4 (phase-2 role):
    0 entry                 1 b1 / X / W1 stages 0, 1 requested     2 behind barrier 0: X + W1 stage 0 usable
    3 behind barrier 1: H of step 0 (32 hidden units) written        4 phase 2 of step 0 issued (its 32 MFMAs are in the pipe)
    5 behind barrier 2: H of step 1 written                          6 phase 2 of the last step issued        7 partial outputs stored
ffn_fused_kernel (csrc/ffn.hip; chunk counts the pipelined form does not take) writes, all from wavefront 0: entry, loads issued,
X + W1_0 usable, H_0 (64 units) done, phase 2 of sub-chunk 0 issued, W1_1 usable, loop done, stored."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cotr_amd import _lib
lib = _lib.load_library()
P = lambda t: None if t is None else t.data_ptr()
sp = _lib.current_stream_ptr()
names = ['entry', 'loads issued', 'X+W1_0 usable', 'H_0 done', 'phase2_0 issued', 'H_1 done', 'loop done', 'stored']
for M in (512, 1000):
    x = torch.randn(M, 256, device='cuda')
    w1, b1 = torch.randn(1024, 256, device='cuda') / 16, torch.randn(1024, device='cuda')
    w2, b2 = torch.randn(256, 1024, device='cuda') / 32, torch.randn(256, device='cuda')
    lw, lb = torch.ones(256, device='cuda'), torch.zeros(256, device='cuda')
    nch = lib.cotr_op_ffn_chunks(M)
    scratch = torch.empty(nch * M * 256, device='cuda')
    y = torch.empty(M, 256, device='cuda')
    times = torch.zeros(4096, 8, dtype=torch.int64, device='cuda')
    run = lambda: lib.cotr_op_ffn_block(P(x), P(w1), P(b1), P(w2), P(b2), P(lw), P(lb), P(scratch), P(y), M, sp)
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    lib.cotr_debug_ffn_times(P(times))
    times.zero_()
    torch.cuda.synchronize()
    assert run() == 0
    torch.cuda.synchronize()
    lib.cotr_debug_ffn_times(None)
    t = times.cpu()
    t = t[t[:, 0] > 0].double()
    t0 = t[:, 0].min()
    line = '  '.join(f'{n} {((t[:, i] - t0) * 0.01)[t[:, i] > 0].mean():5.2f}' for i, n in enumerate(names) if (t[:, i] > 0).any())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        run()
    e1.record()
    torch.cuda.synchronize()
    print(f'M={M} x{nch} chunks, {t.shape[0]} wgs, FFN + ln_reduce {e0.elapsed_time(e1) * 20:.2f} us back-to-back | us since first entry: {line}', flush=True)
