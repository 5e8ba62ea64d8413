"""Which hardware queue does the HIP runtime deal to a stream?  (EXPERIMENTS E3, "Four hardware queues")

    rocprofv3 --kernel-trace --output-format csv -d OUT -o trace -- python3 tools/queue_map.py
    python3 tools/queue_map.py OUT/trace_kernel_trace.csv

The first form runs one fill on the null stream, on 8 normal-priority and on 4 high-priority streams; every stream's
fill has a grid size of its own.  The second form reads the trace and prints the Queue_Id of each."""
import sys

N_NORMAL, N_HIGH, UNIT = 8, 4, 65536


def run():
    import torch
    dev = "cuda:0"
    streams = [torch.cuda.default_stream(dev)]
    streams += [torch.cuda.Stream(device=dev, priority=0) for _ in range(N_NORMAL)]
    streams += [torch.cuda.Stream(device=dev, priority=-1) for _ in range(N_HIGH)]
    bufs = [torch.empty((i + 1) * UNIT, dtype=torch.int32, device=dev) for i in range(len(streams))]
    torch.cuda.synchronize()
    for rep in range(2):
        for s, b in zip(streams, bufs):
            with torch.cuda.stream(s):
                b.fill_(rep)
    torch.cuda.synchronize()


def read(path):
    import collections
    import csv
    queues = collections.defaultdict(set)
    for r in csv.DictReader(open(path)):
        queues[int(r["Grid_Size_X"])].add(r["Queue_Id"])
    kinds = ["null"] + ["normal"] * N_NORMAL + ["high"] * N_HIGH
    for kind, grid in zip(kinds, sorted(queues)):
        print("%-6s stream (grid %7d): queue %s" % (kind, grid, ", ".join(sorted(queues[grid]))))


if __name__ == "__main__":
    read(sys.argv[1]) if len(sys.argv) > 1 else run()
