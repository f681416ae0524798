"""Micro-timing of the training step's tail: what runs after `model(...)`.

  (a) torch.optim.Adam.step() (default settings) against aerognn.optim.Adam.step() on the C3 parameter
      set (the BiStridedMeshGraphNet bench.py builds, random gradients) and on airfoil_mgn's;
  (b) torch's MSE forward + backward against aerognn.train.mse_loss_grad at 1,000,000 x 4 in bf16 and at
      5,000 x 4 in fp32.

The two versions alternate in one process, warmed up, in windows of at least 0.5 s of host clock that
end in a device synchronise (so a window holds whichever of host enqueue and device work is longer);
the figure is the median window's time per call. aerognn.optim.Adam is timed twice, with its
steady-state replay and with `replay = False` (the full partition at every step). agn_adam_step alone
is also timed with HIP events over repeated launches from the optimizer's own table, for its achieved
bytes/s against the 28 B per parameter the update moves (p, m, v read and written, g read, fp32).

  python tools/step_tail_micro.py [--windows 5]            timings; the last line is one JSON object
  python tools/step_tail_micro.py --master                 the C3 parameter set in bf16: torch.optim.Adam on the
      bf16 parameters (what aerognn.optim.Adam runs for them without the flag) against
      aerognn.optim.Adam(master_weights=True), same method; agn_adam_step_master alone against the 30 B per
      parameter it moves (p, g 2 B and w, m, v 4 B read; p, w, m, v written). With --launch-counts: the
      launches of these two
  python tools/step_tail_micro.py --scaled                 the --master measurement in fp16 with a
      aerognn.train.LossScaler attached: torch's step on the fp16 parameters, the master-weight step and
      LossScaler.step(optimizer) + update() alternate in one run; agn_grad_check alone against the 2 B per
      parameter it reads and agn_adam_step_master_scaled alone. With --launch-counts: the launches of the three
  python tools/step_tail_micro.py --launch-counts          kernel launches per call of each tail, from
      rocprofv3 --kernel-trace --stats runs of this file's --child mode (two lengths per tail; the
      difference of the traces' kernel counts over the difference in calls)

Needs the MI355X: there is no fallback.
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "aero-gnn_amd"))

from aerognn import _lib, optim as agn_optim, train as agn_train  # noqa: E402

dev = torch.device("cuda", 0)
C3_KW = dict(processor_size=15, activation_fn="relu", num_hidden_layers_node_processor=2,
             num_hidden_layers_edge_processor=2, hidden_dim_processor=128, num_hidden_layers_node_encoder=2,
             hidden_dim_node_encoder=128, num_hidden_layers_edge_encoder=2, hidden_dim_edge_encoder=128,
             aggregation="add", hidden_dim_decoder=128, num_hidden_layers_decoder=2, dropout=0.0,
             do_concat_trick=True, num_scales=4, layers_per_scale=2, stride=2)  # bench.py build_model(4)


def param_shapes(which):
    """Shapes of the model's parameters (the models are built on the host; only shapes are used)."""
    torch.manual_seed(0)
    if which == "c3":
        from models.bsms_mgn import BiStridedMeshGraphNet
        m = BiStridedMeshGraphNet(6, 4, 4, **C3_KW)
    else:
        from models.mgn import MeshGraphNet
        with open(os.path.join(ROOT, "tests", "golden", "config_experiments.json")) as f:
            e = json.load(f)["airfoil_mgn"]
        g, (d_n, d_e, d_out) = e["kwargs"].get, e["dims"]
        m = MeshGraphNet(input_node_dim=d_n, input_edge_dim=d_e, output_node_dim=d_out,
                         processor_size=g("processor_size"), activation_fn=g("activation_fn"),
                         num_hidden_layers_node_processor=g("num_hidden_layers_node_processor"),
                         num_hidden_layers_edge_processor=g("num_hidden_layers_edge_processor"),
                         hidden_dim_processor=g("hidden_dim"),
                         num_hidden_layers_node_encoder=g("num_hidden_layers_node_encoder"),
                         hidden_dim_node_encoder=g("hidden_dim"),
                         num_hidden_layers_edge_encoder=g("num_hidden_layers_edge_encoder"),
                         hidden_dim_edge_encoder=g("hidden_dim"), aggregation=g("aggregation"),
                         hidden_dim_decoder=g("hidden_dim"), num_hidden_layers_decoder=g("num_hidden_layers_decoder"),
                         do_concat_trick=g("do_concat_trick"))
    return [tuple(p.shape) for p in m.parameters()]


def make_optimizer(cls, shapes, dtype=torch.float32, **kw):
    g = torch.Generator(device=dev).manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g).to(dtype)) for s in shapes]
    for p in ps:
        p.grad = (torch.randn(p.shape, device=dev, generator=g) * 1e-2).to(dtype)
    return cls(ps, lr=1e-3, **kw), ps


def windows(fns, nwin, min_s=0.5):
    """Median seconds per call of each fn: alternating windows of >= min_s that end in a synchronise."""
    reps = []
    for f in fns:
        for _ in range(5):
            f()
        torch.cuda.synchronize()
        k = 8
        while True:  # calls per window, from a timed trial
            t0 = time.perf_counter()
            for _ in range(k):
                f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= 0.05:
                break
            k *= 4
        reps.append(max(8, int(k * min_s / dt * 1.1) + 1))
    out = [[] for _ in fns]
    for _ in range(nwin):
        for i, f in enumerate(fns):
            while True:
                t0 = time.perf_counter()
                for _ in range(reps[i]):
                    f()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= min_s:
                    break
                reps[i] = int(reps[i] * 1.5) + 1
            out[i].append(dt / reps[i])
    return [statistics.median(o) for o in out], [(min(o), max(o)) for o in out]


def kernel_only(opt, iters=200, dtype=torch.float32):
    """ms per launch of agn_adam_step (agn_adam_step_master for a 16-bit table) from the optimizer's table
    of `dtype` (HIP events)."""
    tab = [t for t in opt._agn_tables.values() if t.dtype == dtype][0]
    lib = _lib.lib()
    fn = lib.agn_adam_step_master if tab.master else lib.agn_adam_step
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        rc = fn(tab.dev.data_ptr(), tab.nt, tab.cmap.data_ptr(), tab.nchunk, tab.code, st)
        assert rc == 0, rc
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, tab.nchunk


def scaled_step(opt):
    """LossScaler.step(opt) + update(): what train() runs in optimizer.step()'s place. The growth interval is
    out of reach, so the scale stays where it starts however long the windows run."""
    scaler = agn_train.LossScaler(dev, growth_interval=2 ** 30)

    def step():
        scaler.step(opt)
        scaler.update()
    return step, scaler


def scaled_kernels(opt, scaler, iters=200, dtype=torch.float16):
    """ms per launch of agn_grad_check and of the scaled Adam kernel from the optimizer's table of `dtype`."""
    tab = [t for t in opt._agn_tables.values() if t.dtype == dtype][0]
    lib = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sp = scaler._device_state().data_ptr()
    args = (tab.dev.data_ptr(), tab.nt, tab.cmap.data_ptr(), tab.nchunk, tab.code)
    step = lib.agn_adam_step_master_scaled if tab.master else lib.agn_adam_step_scaled

    def check():
        rc = lib.agn_grad_check(args[0], int(tab.master), *args[1:], sp, st)
        assert rc == 0, rc

    def adam():
        rc = step(*args, sp, st)
        assert rc == 0, rc
    out = []
    for run in (check, adam):
        for _ in range(10):
            run()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            run()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters)
    return out


def mse_pair(n, f, dtype):
    g = torch.Generator(device=dev).manual_seed(2)
    pred = torch.randn(n, f, device=dev, generator=g).to(dtype).requires_grad_(True)
    y = torch.randn(n, f, device=dev, generator=g).to(dtype)
    loss_fn = torch.nn.MSELoss()

    def torch_tail():
        pred.grad = None
        loss_fn(pred, y).backward()

    def ours():
        agn_train.mse_loss_grad(pred, y)
    return torch_tail, ours


def tails():
    """name -> a callable that builds (and returns) one tail's step function."""
    def adam(cls, which, dtype=torch.float32, **kw):
        def build():
            opt, _ = make_optimizer(cls, param_shapes(which), dtype, **kw)
            return opt.step
        return build

    def scaled(which, dtype):
        def build():
            opt, _ = make_optimizer(agn_optim.Adam, param_shapes(which), dtype, master_weights=True)
            return scaled_step(opt)[0]
        return build

    def mse(n, f, dtype, i):
        return lambda: mse_pair(n, f, dtype)[i]
    return {"adam_torch_c3": adam(torch.optim.Adam, "c3"), "adam_ours_c3": adam(agn_optim.Adam, "c3"),
            "adam_torch_airfoil": adam(torch.optim.Adam, "airfoil"), "adam_ours_airfoil": adam(agn_optim.Adam, "airfoil"),
            "adam_torch_c3_bf16": adam(torch.optim.Adam, "c3", torch.bfloat16),
            "adam_master_c3_bf16": adam(agn_optim.Adam, "c3", torch.bfloat16, master_weights=True),
            "adam_torch_c3_f16": adam(torch.optim.Adam, "c3", torch.float16),
            "adam_master_c3_f16": adam(agn_optim.Adam, "c3", torch.float16, master_weights=True),
            "adam_scaled_c3_f16": scaled("c3", torch.float16),
            "mse_torch_5000x4_f32": mse(5000, 4, torch.float32, 0), "mse_ours_5000x4_f32": mse(5000, 4, torch.float32, 1),
            "mse_torch_1Mx4_bf16": mse(1000000, 4, torch.bfloat16, 0), "mse_ours_1Mx4_bf16": mse(1000000, 4, torch.bfloat16, 1)}


def child(name, calls):
    f = tails()[name]()
    for _ in range(calls):
        f()
    torch.cuda.synchronize()


def count_kernels(name, calls, tmp):
    d = os.path.join(tmp, f"{name}_{calls}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
           sys.executable, os.path.abspath(__file__), "--child", name, "--calls", str(calls)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {d}"
    n = 0
    for fn in files:
        with open(fn, newline="") as fh:
            n += sum(1 for _ in csv.DictReader(fh))
    return n


def launch_counts(names):
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            a, b = count_kernels(name, 4, tmp), count_kernels(name, 12, tmp)
            res[name] = (b - a) / 8.0
            print(f"{name:28s} {res[name]:8.2f} kernel launches per call ({a} at 4 calls, {b} at 12)", flush=True)
    return res


def master(nwin):
    """The C3 parameter set in bf16: torch's step on the bf16 parameters against the master-weight step."""
    shapes = param_shapes("c3")
    nparam = sum(int(torch.Size(s).numel()) for s in shapes)
    ot, _ = make_optimizer(torch.optim.Adam, shapes, torch.bfloat16)
    om, _ = make_optimizer(agn_optim.Adam, shapes, torch.bfloat16, master_weights=True)
    (tt, tm), spread = windows([ot.step, om.step], nwin)
    kms, nchunk = kernel_only(om, dtype=torch.bfloat16)
    gbs = 30.0 * nparam / (kms * 1e-3) / 1e9
    res = {"adam_master_c3_bf16": {"tensors": len(shapes), "params": nparam, "torch_bf16_us": tt * 1e6, "master_us": tm * 1e6,
                                   "torch_over_master": tt / tm, "torch_minmax_us": [x * 1e6 for x in spread[0]],
                                   "master_minmax_us": [x * 1e6 for x in spread[1]], "kernel_us": kms * 1e3,
                                   "kernel_GBps": gbs, "chunks": nchunk}}
    print(f"adam c3 bf16: {len(shapes)} tensors, {nparam} parameters: torch on the bf16 parameters {tt * 1e6:.1f} us/step, "
          f"master weights {tm * 1e6:.1f} us/step (x{tt / tm:.2f}); agn_adam_step_master alone {kms * 1e3:.1f} us = "
          f"{gbs:.0f} GB/s of 30 B/parameter ({nchunk} chunks)", flush=True)
    print(json.dumps(res), flush=True)


def scaled(nwin):
    """The C3 parameter set in fp16: torch's step, the master-weight step and the loss-scaled step."""
    shapes = param_shapes("c3")
    nparam = sum(int(torch.Size(s).numel()) for s in shapes)
    ot, _ = make_optimizer(torch.optim.Adam, shapes, torch.float16)
    om, _ = make_optimizer(agn_optim.Adam, shapes, torch.float16, master_weights=True)
    os_, _ = make_optimizer(agn_optim.Adam, shapes, torch.float16, master_weights=True)
    step, scaler = scaled_step(os_)
    (tt, tm, ts), spread = windows([ot.step, om.step, step], nwin)
    assert scaler.steps_skipped() == 0
    kms, nchunk = kernel_only(om, dtype=torch.float16)
    cms, sms = scaled_kernels(os_, scaler)
    res = {"adam_scaled_c3_f16": {"tensors": len(shapes), "params": nparam, "torch_f16_us": tt * 1e6, "master_us": tm * 1e6,
                                  "scaled_us": ts * 1e6, "scaled_over_master": ts / tm, "torch_over_scaled": tt / ts,
                                  "torch_minmax_us": [x * 1e6 for x in spread[0]],
                                  "master_minmax_us": [x * 1e6 for x in spread[1]],
                                  "scaled_minmax_us": [x * 1e6 for x in spread[2]], "master_kernel_us": kms * 1e3,
                                  "check_kernel_us": cms * 1e3, "check_GBps": 2.0 * nparam / (cms * 1e-3) / 1e9,
                                  "scaled_kernel_us": sms * 1e3, "chunks": nchunk}}
    print(f"adam c3 fp16: {len(shapes)} tensors, {nparam} parameters: torch on the fp16 parameters {tt * 1e6:.1f} us/step, "
          f"master weights {tm * 1e6:.1f} us/step, LossScaler.step + update {ts * 1e6:.1f} us/step (x{ts / tm:.2f} of the "
          f"master step, torch x{tt / ts:.2f}); kernels alone: agn_adam_step_master {kms * 1e3:.1f} us, "
          f"agn_adam_step_master_scaled {sms * 1e3:.1f} us, agn_grad_check {cms * 1e3:.1f} us = "
          f"{2.0 * nparam / (cms * 1e-3) / 1e9:.0f} GB/s of 2 B/parameter ({nchunk} chunks)", flush=True)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launch-counts", action="store_true")
    ap.add_argument("--master", action="store_true")
    ap.add_argument("--scaled", action="store_true")
    ap.add_argument("--child")
    ap.add_argument("--calls", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("step_tail_micro needs the MI355X (no fallback)")
    if a.child:
        return child(a.child, a.calls)
    if a.launch_counts:
        group = "_c3_f16" if a.scaled else "_c3_bf16" if a.master else ""
        names = [n for n in sorted(tails()) if (n.endswith(group) if group else not n.endswith(("_c3_bf16", "_c3_f16")))]
        print(json.dumps({"launches_per_call": launch_counts(names)}), flush=True)
        return
    if a.scaled:
        return scaled(a.windows)
    if a.master:
        return master(a.windows)
    res = {}
    for which in ("c3", "airfoil"):
        shapes = param_shapes(which)
        nparam = sum(int(torch.Size(s).numel()) for s in shapes)
        ot, _ = make_optimizer(torch.optim.Adam, shapes)
        oo, _ = make_optimizer(agn_optim.Adam, shapes)
        on, _ = make_optimizer(agn_optim.Adam, shapes)
        on.replay = False  # the full partition at every step: what the steady-state replay saves
        (tt, to, tn), spread = windows([ot.step, oo.step, on.step], a.windows)
        kms, nchunk = kernel_only(oo)
        gbs = 28.0 * nparam / (kms * 1e-3) / 1e9
        res[f"adam_{which}"] = {"tensors": len(shapes), "params": nparam, "torch_us": tt * 1e6, "ours_us": to * 1e6,
                               "ours_no_replay_us": tn * 1e6, "torch_over_ours": tt / to, "torch_minmax_us": [x * 1e6 for x in spread[0]],
                               "ours_minmax_us": [x * 1e6 for x in spread[1]], "kernel_us": kms * 1e3,
                               "kernel_GBps": gbs, "chunks": nchunk}
        print(f"adam {which}: {len(shapes)} tensors, {nparam} parameters: torch {tt * 1e6:.1f} us/step, ours "
              f"{to * 1e6:.1f} us/step (x{tt / to:.2f}), without the replay {tn * 1e6:.1f} us/step; agn_adam_step alone {kms * 1e3:.1f} us = {gbs:.0f} GB/s of "
              f"28 B/parameter ({nchunk} chunks)", flush=True)
    for n, f, dtype, tag in ((1000000, 4, torch.bfloat16, "1Mx4_bf16"), (5000, 4, torch.float32, "5000x4_f32")):
        ft, fo = mse_pair(n, f, dtype)
        (tt, to), spread = windows([ft, fo], a.windows)
        res[f"mse_{tag}"] = {"torch_us": tt * 1e6, "ours_us": to * 1e6, "torch_over_ours": tt / to,
                             "torch_minmax_us": [x * 1e6 for x in spread[0]], "ours_minmax_us": [x * 1e6 for x in spread[1]]}
        print(f"mse {tag}: torch forward + backward {tt * 1e6:.1f} us, mse_loss_grad {to * 1e6:.1f} us (x{tt / to:.2f})",
              flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
