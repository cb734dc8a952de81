"""run_gnn_trackml_mod.sh (:7-146) as one process: event conversion and iterations
START..END of clustering / extrapolation -> candidate extraction -> metadata update,
every stage on the GPU (gtf.pipeline), stage outputs saved in the compact packed
format (gtf.store) instead of per-subgraph gpickles.

    python run_pipeline.py -n <event_network dir> -o <ROOTDIR> -a 7 -z 7 [--start 1 --end 3]

Layout under ROOTDIR (the run script's directories, one file each):

    track_sim/network/graph.npz              event conversion output
    iteration_i/network/graph.npz            the iteration's stage output
    iteration_i/candidates/candidates.npz    extracted candidates (node ids) + p-values
    iteration_i/candidates/pvals.csv         as extract_track_candidates.py writes it (:485-486)
    iteration_i/remaining/graph.npz          the next iteration's input (after update on even i)
    iteration_i/fragments/fragments.npz      node ids of the track fragments
    timings.json                             wall time per stage
    metrics.json                             with --truth: reconstruction efficiency and purities
                                             (gtf.metrics; the run script's last step, :143-146)

--resident / --resident-outputs keep the graph between iterations on the GPU; --resident-event also
builds the event there (pipeline.build_event_dev) and starts iteration 1 on that object. Same files.
--resident-metrics (implies --resident-outputs) scores the candidates on the GPU as well: with --truth,
metrics.json comes from gtf.metrics.DeviceScorer, fed each iteration's candidates where
gtf_extract_outputs left them, instead of from the saved lists. The same values.
--resident-truth (implies --resident-metrics) also builds the scorer's truth tables on the GPU
(gtf.metrics.truth_tables_dev) from the parsed truth files. The same metrics.json, byte for byte.
--resident-parse (implies --resident-event) also parses the event's CSV files on the GPU (gtf_csv_parse;
pipeline.build_event_dev(parse="device")) and, with --resident-truth, the truth files
(gtf.metrics.truth_files_dev). One line per file says which parser read it: a file with a field outside
the device parser's exact domain is read by the host reader. The same files either way.

--batch DIR [DIR ...] takes several --eventNetwork directories at once: every event is built in GPU memory
(as --resident-event), the events are fused (DeviceGraph.concat) and the loop runs once on the fused graph
(pipeline.run_batch); with --truth (one directory for every event, or one per event) the candidates are
scored on the GPU as with --resident-metrics. Event i's files go under ROOTDIR/<i>/ in the layout above, the
same files a single run of that event writes. If a stage raises a reference exception the whole batch
stops (--batch-on-error raise, the default; name: the message names the failing events). With
--batch-on-error isolate the failing events are cut out of the fused graph (pipeline.run_batch(on_error=
"isolate")): ROOTDIR/<i>/ of a failed event holds its clean iterations and error.json (iteration, stage,
flags, messages, node_id, n_raising) and no metrics.json, one line says so, the other events' files are
those of the same command without the failing directories, and the exit status is 0.
--batch-build (with --batch) builds the events in ONE call (pipeline.build_events_dev:
gtf_build_events_csr_device on the concatenated columns) instead of once per event followed by the concat:
the same files under ROOTDIR/<i>/.
--batch-metrics (with --batch and --truth) scores the whole batch with ONE pair of scorers
(gtf.metrics.BatchScorer: gtf_score_candidates_ev once per iteration on the fused graph's candidates) instead
of a pair per event; the truth tables are still made per event and then concatenated. The same metrics.json
under every ROOTDIR/<i>/, byte for byte.
--batch-truth (with --batch-metrics) makes the truth tables of the whole batch in ONE build as well
(gtf.metrics.truth_tables_batch_dev: gtf_truth_build_ev on the events' columns laid end to end; with
--resident-parse the truth files are parsed on the GPU first, per file). The same metrics.json files.
--batch-parse (with --batch-build and --resident-parse) parses the batch's CSV files per kind instead of
per file: all nodes.csv in ONE gtf_csv_parse_ev, one window and one radius patch, all edges.csv in one more
parse (pipeline.build_events_dev(batch_parse=True)); with --batch-truth the particles, mapping and truth
files too (gtf.metrics.truth_files_batch_dev(batch_parse=True)). The same files under every ROOTDIR/<i>/.

--start S > 1 resumes from ROOTDIR/iteration_{S-1}/remaining/graph.npz, as the run
script's commented "iteration by iteration" mode does (:79-81).
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from gtf import extract, pipeline, store  # noqa: E402
from gtf.params import Params  # noqa: E402


def _dir(*parts):
    d = os.path.join(*parts)
    os.makedirs(d, exist_ok=True)
    return d


class _Scorers:
    """what pipeline.run(scorer=...) feeds: one DeviceScorer over every iteration ("cumulative") and
    one that holds the latest iteration only ("last_iteration", as the run script leaves the
    directory): it is reset before each add"""

    def __init__(self, tables, device):
        from gtf import metrics
        self.cumulative = metrics.DeviceScorer(tables, device)
        self.last = metrics.DeviceScorer(tables, device)

    def add(self, cand_ptr, cand_ids, n_cand, group, **kw):
        self.cumulative.add(cand_ptr, cand_ids, n_cand, group, **kw)
        self.last.reset()
        self.last.add(cand_ptr, cand_ids, n_cand, 0, **kw)


def _parser_line(key, info):
    print("parse %s: %s%s" % (key, info[key], " (%s)" % info[key + "_reason"] if key + "_reason" in info else ""))


class _BatchScorers:
    """_Scorers for a whole batch (--batch-metrics): what pipeline.run_batch(scorers=...) feeds once per
    iteration; the last-iteration scorer resets the events that entered the iteration with nodes"""

    def __init__(self, tables, device):
        """tables: one entry per event (truth_concat_dev's), or the batch's DeviceTruthBatch (--batch-truth)"""
        from gtf import metrics
        batch = tables if isinstance(tables, metrics.DeviceTruthBatch) else metrics.truth_concat_dev(tables, device)
        self.cumulative = metrics.BatchScorer(batch)
        self.last = metrics.BatchScorer(batch)

    def add_batch(self, cand_ptr, cand_ids, cand_first, n_cand, group, n_members=None, active=None):
        self.cumulative.add_batch(cand_ptr, cand_ids, cand_first, n_cand, group, n_members=n_members, active=active)
        self.last.reset(events=active)
        self.last.add_batch(cand_ptr, cand_ids, cand_first, n_cand, 0, n_members=n_members, active=active)

    def per_event(self):
        """-> per event an object with _Scorers' two members, each holding its finished Result"""
        import types
        done = lambda r: types.SimpleNamespace(result=lambda: r)   # noqa: E731
        return [None if c is None else types.SimpleNamespace(cumulative=done(c), last=done(l))
                for c, l in zip(self.cumulative.results(), self.last.results())]


def _scorers(args, truth_dir=None):
    """the truth files as reconstruction_efficiency.score reads them -> the two device scorers"""
    return _Scorers(_tables(args, truth_dir), args.device)


def _truth_columns(args, pre):
    """the truth files as reconstruction_efficiency.score reads them, by the host reader -> (HitMapping,
    particle_id, px, py, truth hit_id or None, truth particle_id or None)"""
    import numpy as np
    import pandas as pd
    from gtf import metrics
    particles = pd.read_csv(pre + "particles.csv")
    m = metrics.HitMapping.from_frame(pd.read_csv(pre + args.mapping))
    th = tp = None
    if os.path.isfile(pre + "truth.csv"):
        truth = pd.read_csv(pre + "truth.csv", usecols=["hit_id", "particle_id"])
        th, tp = truth.hit_id.to_numpy(np.int64), truth.particle_id.to_numpy(np.int64)
    return m, particles.particle_id.to_numpy(), particles.px.to_numpy(), particles.py.to_numpy(), th, tp


def _tables_batch(args, truth):
    """--batch-truth: the truth tables of the whole batch from ONE build (gtf.metrics.truth_tables_batch_dev;
    with --resident-parse the files are parsed on the GPU, per file: truth_files_batch_dev); truth: one
    directory per event, None = an event without truth"""
    from gtf import metrics
    pres = [os.path.join(t, "event000001000-") if t else None for t in truth]
    if args.resident_parse:
        batch, infos = metrics.truth_files_batch_dev(pres, args.mapping, args.min_volume, args.max_volume, args.device,
                                                     batch_parse=args.batch_parse)
        for i, info in enumerate(infos):
            for key in ("particles", "mapping", "truth"):
                if info and key in info:
                    print("event %d " % i, end="")
                    _parser_line(key, info)
        return batch
    parts = []
    for pre in pres:
        if pre is None:
            parts.append(None)
            continue
        m, pid, px, py, th, tp = _truth_columns(args, pre)
        parts.append((m, pid, px, py) + ((th, tp) if th is not None else ()))
    return metrics.truth_tables_batch_dev(parts, args.min_volume, args.max_volume, args.device)


def _tables(args, truth_dir=None):
    """the truth files as reconstruction_efficiency.score reads them -> the scorer's truth tables"""
    from gtf import metrics
    pre = os.path.join(truth_dir or args.truth, "event000001000-")
    if args.resident_parse and args.resident_truth:
        tables, info = metrics.truth_files_dev(pre, args.mapping, args.min_volume, args.max_volume, args.device)
        for key in ("particles", "mapping", "truth"):
            if key in info:
                _parser_line(key, info)
        return tables
    m, pid, px, py, th, tp = _truth_columns(args, pre)
    cols = (m, pid, px, py, args.min_volume, args.max_volume, th, tp)
    if args.resident_truth:
        tables = metrics.truth_tables_dev(*cols, device=args.device)
    else:
        tables = metrics.truth_tables(*cols)
    return tables


def main(argv=None):
    ap = argparse.ArgumentParser(description="GNN track finding on the GPU (run_gnn_trackml_mod.sh)")
    ap.add_argument("-n", "--eventNetwork", help="directory holding event_1_filtered_graph_{nodes,edges}.csv")
    ap.add_argument("-o", "--outputDir", required=True, help="ROOTDIR")
    ap.add_argument("-a", "--min_volume", type=int, default=7)
    ap.add_argument("-z", "--max_volume", type=int, default=7)
    ap.add_argument("-e", "--sigma0xy", type=float, default=0.3)
    ap.add_argument("-r", "--sigma0rz", type=float, default=0.4)
    ap.add_argument("-m", "--sigma0rz2", type=float, default=0.6)
    ap.add_argument("-b", "--endcapboundary", type=float, default=550.0)
    ap.add_argument("-c", "--chi2", type=float, default=2.0, help="extrapolation chi2 cut (c)")
    ap.add_argument("-p", "--pval", type=float, default=0.01)
    ap.add_argument("--numhits", type=int, default=4, help="n")
    ap.add_argument("-s", "--separation", type=float, default=10.0)
    ap.add_argument("-t", "--merge", type=float, default=8.0, help="threshold distance node merging")
    ap.add_argument("--start", type=int, default=1)
    ap.add_argument("--end", type=int, default=3)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--resident", action="store_true",
                    help="cut each iteration's remaining graph on the GPU (DeviceGraph.subset) instead of on the host")
    ap.add_argument("--resident-outputs", action="store_true",
                    help="as --resident, and the candidate order and the stage outputs are computed on the GPU too "
                         "(pipeline.run(resident='device')): only the id lists and p-values come back")
    ap.add_argument("--resident-event", action="store_true",
                    help="as --resident-outputs, and event conversion builds the event in GPU memory "
                         "(pipeline.build_event_dev): iteration 1 starts on that object; only with --start 1")
    ap.add_argument("--resident-metrics", action="store_true",
                    help="as --resident-outputs, and with --truth the candidates are scored on the GPU "
                         "(gtf.metrics.DeviceScorer) from the extraction's device arrays; only with --start 1")
    ap.add_argument("--resident-truth", action="store_true",
                    help="as --resident-metrics, and the scorer's truth tables are built on the GPU too "
                         "(gtf.metrics.truth_tables_dev); only with --start 1")
    ap.add_argument("--resident-parse", action="store_true",
                    help="as --resident-event, and the CSV files are parsed on the GPU (gtf_csv_parse); with "
                         "--resident-truth the truth files as well; only with --start 1")
    ap.add_argument("--batch", nargs="+", metavar="DIR",
                    help="several event_network directories: the events are built in GPU memory, fused and run as one "
                         "loop (pipeline.run_batch); event i's outputs go under ROOTDIR/<i>/; only with --start 1")
    ap.add_argument("--batch-build", action="store_true",
                    help="with --batch: one graph build for all events (pipeline.build_events_dev) instead of one "
                         "per event and a concat; the same files")
    ap.add_argument("--batch-on-error", choices=("raise", "name", "isolate"), default="raise",
                    help="with --batch: what a reference exception in one event does (pipeline.run_batch(on_error=)): "
                         "raise: the whole batch stops, as before; name: it stops and the message names the failing "
                         "events; isolate: the failing events are cut out, their ROOTDIR/<i>/ holds their clean "
                         "iterations and an error.json (no metrics.json), the others finish and the exit status is 0")
    ap.add_argument("--batch-metrics", action="store_true",
                    help="with --batch and --truth: one pair of scorers for the whole batch (gtf.metrics.BatchScorer: "
                         "one scoring call per iteration) instead of a pair per event; the same metrics.json files")
    ap.add_argument("--batch-truth", action="store_true",
                    help="with --batch-metrics: the truth tables of the whole batch come from one build "
                         "(gtf.metrics.truth_tables_batch_dev) instead of one per event and a concat; the same "
                         "metrics.json files")
    ap.add_argument("--batch-parse", action="store_true",
                    help="with --batch-build and --resident-parse: the CSV files of the batch are parsed per kind in "
                         "one call each (gtf_csv_parse_ev) instead of per file; with --batch-truth the truth files "
                         "too; the same files")
    ap.add_argument("--truth", nargs="+", metavar="DIR",
                    help="EVENT_TRUTH dir: score the candidates (reconstruction_efficiency.py); with --batch one "
                         "directory for every event, or one per event")
    ap.add_argument("--mapping", default="full-mapping-minCurv-0.3-800.csv", help="mapping file under --truth")
    args = ap.parse_args(argv)
    if args.start < 1 or args.end < args.start:
        ap.error("need 1 <= start <= end")
    args.truth_dirs = args.truth or []
    if args.truth_dirs and len(args.truth_dirs) != 1 and (not args.batch or len(args.truth_dirs) != len(args.batch)):
        ap.error("--truth takes one directory (with --batch: one, or one per event)")
    args.truth = args.truth_dirs[0] if args.truth_dirs else None
    if args.batch:
        if args.start != 1:
            ap.error("--batch converts the events: only with --start 1")
        if args.eventNetwork:
            ap.error("--batch names the event directories itself: not with -n")
    if args.batch_build and not args.batch:
        ap.error("--batch-build builds the events of --batch")
    if args.batch_on_error != "raise" and not args.batch:
        ap.error("--batch-on-error is a policy of --batch")
    if args.batch_metrics and not (args.batch and args.truth_dirs):
        ap.error("--batch-metrics scores the events of --batch against --truth")
    if args.batch_truth and not args.batch_metrics:
        ap.error("--batch-truth builds the truth tables of --batch-metrics")
    if args.batch_parse and not (args.batch_build and args.resident_parse):
        ap.error("--batch-parse parses the files of --batch-build --resident-parse")
    if args.resident_parse:
        args.resident_event = True
    if args.resident_event and args.start != 1:
        ap.error("--resident-event converts the event: only with --start 1")
    if args.resident_truth:
        args.resident_metrics = True
    if args.resident_metrics and args.start != 1:
        ap.error("--resident-metrics scores the iterations of this run: only with --start 1")
    p = Params(sigma0xy=args.sigma0xy, sigma0rz=args.sigma0rz, sigma0rz2=args.sigma0rz2,
               endcap_boundary=args.endcapboundary, chi2_cut=args.chi2)
    ex = extract.Params(args.pval, args.numhits, args.separation, args.merge, args.sigma0xy, args.sigma0rz,
                        args.endcapboundary)
    if args.batch:
        return _batch(args, p, ex)
    root = args.outputDir
    times = {}
    if args.start == 1:
        if not args.eventNetwork:
            ap.error("-n is required when starting at iteration 1")
        t0 = time.perf_counter()
        prefix = os.path.join(args.eventNetwork, "event_1_filtered_graph_")
        if args.resident_event:
            dev = pipeline.build_event_dev(prefix, args.min_volume, args.max_volume, p, args.device,
                                           parse="device" if args.resident_parse else "host")
            if args.resident_parse:
                for key in ("nodes", "edges"):
                    _parser_line(key, dev.parse_info)
            g, vivl = dev.host_graph()   # (the saved file; the loop starts on the resident object)
        else:
            g, vivl = pipeline.build_event(prefix, args.min_volume, args.max_volume, p, args.device)
        times["event_conversion"] = time.perf_counter() - t0
        store.save_graph(os.path.join(_dir(root, "track_sim", "network"), "graph.npz"), g, vivl)
        print("event conversion: %d nodes, %d directed edges, %d subgraphs (%.3f s)"
              % (g.n_nodes, g.n_edges, g.n_subgraphs, times["event_conversion"]))
    else:
        g, vivl = store.load_graph(os.path.join(root, "iteration_%d" % (args.start - 1), "remaining", "graph.npz"))
        if vivl is None:
            raise SystemExit("remaining graph has no vivl array")
    scorers = _scorers(args) if args.resident_metrics and args.truth else None
    extra = {"scorer": scorers} if scorers else {}
    if args.resident_event and g.n_nodes:
        its = pipeline.run(dev, None, args.end - args.start + 1, p, ex, args.device, first=1, keep_graphs=True,
                           resident="device", host=g, **extra)   # (the download above: no second one)
    else:
        on_dev = args.resident_outputs or args.resident_event or args.resident_metrics
        its = pipeline.run(g, vivl, args.end - args.start + 1, p, ex, args.device, first=args.start, keep_graphs=True,
                           resident="device" if on_dev else args.resident, **extra)
    _save(root, its, times)
    _metrics(args, root, its, scorers, args.truth)
    return 0


def _save(root, its, times):
    """the iterations' files and timings.json under root"""
    for it in its:
        d = os.path.join(root, "iteration_%d" % it.index)
        store.save_graph(os.path.join(_dir(d, "network"), "graph.npz"), it.network)
        cdir = _dir(d, "candidates")
        store.save_groups(os.path.join(cdir, "candidates.npz"), it.candidates, pval_xy=it.pval_xy,
                          pval_zr=it.pval_zr)
        with open(os.path.join(cdir, "pvals.csv"), "w") as f:
            f.write(",pvals_xy,pvals_zr\n")
            for i, (a, b) in enumerate(zip(it.pval_xy, it.pval_zr)):
                f.write("%d,%r,%r\n" % (i, float(a), float(b)))
        store.save_graph(os.path.join(_dir(d, "remaining"), "graph.npz"), it.remaining_graph, it.remaining_vivl)
        store.save_groups(os.path.join(_dir(d, "fragments"), "fragments.npz"), it.fragments)
        times["iteration_%d" % it.index] = it.seconds
        print("iteration %d (%s): %d candidates, %d remaining, %d fragments"
              % (it.index, it.stage, len(it.candidates), len(it.remaining), len(it.fragments)))
    with open(os.path.join(_dir(root), "timings.json"), "w") as f:
        json.dump(times, f, indent=1)


def _metrics(args, root, its, scorers, truth_dir):
    """metrics.json under root: from the device scorers, else from the saved lists"""
    if truth_dir and its:
        from extract import reconstruction_efficiency as re_cli
        from gtf import metrics
        res = {}
        for name, cum in (("last_iteration", False), ("cumulative", True)):
            if scorers:
                r = (scorers.cumulative if cum else scorers.last).result()
            else:
                r = re_cli.score(truth_dir, root, args.min_volume, args.max_volume, its[-1].index, args.mapping, cum)
            res[name] = metrics.summary(r)
            print("%s: %d / %d reference tracks reconstructed, efficiency %s %%"
                  % (name, r.n_reconstructed, r.n_reference, r.efficiency_str))
        with open(os.path.join(root, "metrics.json"), "w") as f:
            json.dump(res, f, indent=1)


def _batch(args, p, ex):
    """--batch: the events built in GPU memory, one fused loop, event i's files under ROOTDIR/<i>/"""
    devs, times = [], []
    if args.batch_build:
        import numpy as np
        from gtf.graph import split_events
        t0 = time.perf_counter()
        fused = pipeline.build_events_dev([os.path.join(dn, "event_1_filtered_graph_") for dn in args.batch],
                                          args.min_volume, args.max_volume, p, args.device,
                                          parse="device" if args.resident_parse else "host",
                                          batch_parse=args.batch_parse, on_error=args.batch_on_error)
        if args.resident_parse:
            for info in fused.parse_info:
                for key in ("nodes", "edges"):
                    _parser_line(key, info)
        G, vivl = fused.host_graph()
        event = fused._np(fused.carried["event"])
        cut = np.searchsorted(event, np.arange(len(args.batch) + 1))
        seconds = (time.perf_counter() - t0) / max(len(args.batch), 1)   # (one build: every event its share)
        for i, g in enumerate(split_events(G, event, len(args.batch))):
            times.append({"event_conversion": seconds})
            store.save_graph(os.path.join(_dir(args.outputDir, str(i), "track_sim", "network"), "graph.npz"), g,
                             vivl[cut[i]:cut[i + 1]])
            print("event %d conversion: %d nodes, %d directed edges, %d subgraphs (%.3f s)"
                  % (i, g.n_nodes, g.n_edges, g.n_subgraphs, seconds))
        devs = fused
    for i, dn in enumerate(() if args.batch_build else args.batch):
        t0 = time.perf_counter()
        dev = pipeline.build_event_dev(os.path.join(dn, "event_1_filtered_graph_"), args.min_volume, args.max_volume, p,
                                       args.device, parse="device" if args.resident_parse else "host")
        if args.resident_parse:
            for key in ("nodes", "edges"):
                _parser_line(key, dev.parse_info)
        g, vivl = dev.host_graph()
        times.append({"event_conversion": time.perf_counter() - t0})
        store.save_graph(os.path.join(_dir(args.outputDir, str(i), "track_sim", "network"), "graph.npz"), g, vivl)
        print("event %d conversion: %d nodes, %d directed edges, %d subgraphs (%.3f s)"
              % (i, g.n_nodes, g.n_edges, g.n_subgraphs, times[i]["event_conversion"]))
        devs.append(dev)
    truth = [None] * len(args.batch)
    if args.truth_dirs:
        truth = args.truth_dirs if len(args.truth_dirs) > 1 else args.truth_dirs * len(args.batch)
    if args.batch_metrics:   # one pair of scorers for the batch; the tables per event, or (--batch-truth) in one build
        if args.batch_truth:
            batch = _BatchScorers(_tables_batch(args, truth), args.device)
        else:
            batch = _BatchScorers([_tables(args, t) if t else None for t in truth], args.device)
        its = pipeline.run_batch(devs, args.end - args.start + 1, p, ex, scorers=batch, first=1, keep_graphs=True,
                                 on_error=args.batch_on_error)
        scorers = batch.per_event()
    else:
        scorers = [_scorers(args, t) if t else None for t in truth]
        its = pipeline.run_batch(devs, args.end - args.start + 1, p, ex, scorers=scorers if args.truth_dirs else None,
                                 first=1, keep_graphs=True, on_error=args.batch_on_error)
    errors = dict(getattr(devs, "event_error_records", None) or {})   # (--batch-build: raised in the conversion)
    errors.update(getattr(its, "errors", {}))
    for i, rec in enumerate(its):
        root = os.path.join(args.outputDir, str(i))
        print("event %d:" % i)
        _save(root, rec, times[i])
        if i in errors:   # --batch-on-error isolate: its clean iterations above, no metrics
            err = errors[i]
            with open(os.path.join(root, "error.json"), "w") as f:
                json.dump({"iteration": err.iteration, "stage": err.stage, "flags": err.flags, "messages": err.messages,
                           "node_id": err.first_node_id, "n_raising": err.n_raising}, f, indent=1)
            print("event %d failed in iteration %d (%s): %s; node id %d"
                  % (i, err.iteration, err.stage, "; ".join(err.messages), err.first_node_id))
            continue
        _metrics(args, root, rec, scorers[i], truth[i])
    return 0


if __name__ == "__main__":
    sys.exit(main())
