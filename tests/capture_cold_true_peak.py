"""Run in a FRESH process by tests/test_gpu_r128.py::test_true_peak_is_capturable_as_the_first_call_of_a_process: the process' first call
into the library is a true_peak under stream capture (the taps travel as kernel arguments, no table is uploaded)."""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
import l3ac_amd
g = torch.Generator().manual_seed(5)
x = (0.4 * torch.randn(3, 4 * 1024 + 77, generator=g)).cuda()
lens = [4 * 1024 + 77, 1025, 20]
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    with torch.cuda.graph(graph, stream=s):  # the FIRST library call of the process
        got = l3ac_amd.true_peak(x, 8000, lengths=lens)
graph.replay()
torch.cuda.synchronize()
eager = l3ac_amd.true_peak(x, 8000, lengths=lens)
same = all(torch.equal(got[k], eager[k]) for k in ("true_peak", "true_peak_db", "peak"))
above = bool((eager["true_peak"] >= eager["peak"]).all() and (eager["peak"] > 0).all())
x.mul_(0.5)  # the replay reads the tensor's current contents
graph.replay()
torch.cuda.synchronize()
halved = torch.equal(got["true_peak"] * 2.0, eager["true_peak"])
print("captured as the first call; bits equal", same, "true peak above the peak", above, "replay follows the input", halved)
