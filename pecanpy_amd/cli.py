"""``pecanpy`` command line on the MI355X walk engine.

Flag names, defaults, the mode sanity rules and the stage order follow the reference CLI
(src/pecanpy/cli.py: flags :27-176, ``check_mode`` :179-254, ``read_graph`` :257-304, pipeline
:307-351) so that existing invocations keep working.  Walks come from the GPU; the skip-gram stage
uses gensim when it is importable; without it walks and skip-gram both run on the GPU (``Base.embed_array``: the
walk matrix stays in device memory).  ``--task walks`` writes the walks (one per line) to ``--output`` instead of training,
the text made in device memory; ``PECANPY_AMD_DUMP_WALKS=1`` does the same through the ID lists of ``simulate_walks``.
``--task train`` takes such a file as ``--input`` and trains from it on the GPU, without a graph.
``--task neighbours`` takes an embedding file as ``--input`` and writes the nearest neighbours of its nodes (``embed.KnnIndex``).
``--task score`` takes an embedding file as ``--input`` and writes the score of every pair of ``--pairs``; with ``--neg_pairs`` it
also prints the exact AUC of the two sets of scores (``linkpred``).
``--task split`` holds out a seeded share of the graph's edges on the GPU (``Base.holdout_edges``): the train graph goes to
``--output`` as a CSR ``.npz``, the held-out pairs to ``--pairs`` and, with ``--neg_pairs``, as many non-edges of the original graph
there -- the files ``--task score`` reads.  ``split``, a normal run on the train ``.npz``, ``score``: the link-prediction protocol.
``--task baseline`` scores the pairs of ``--pairs`` by a neighbourhood heuristic of the graph given as ``--input`` (``--heuristic``:
common neighbours, Jaccard, Adamic-Adar, resource allocation, preferential attachment; ``Base.neighbour_scores``) and, with
``--neg_pairs``, prints the same ``auc wins ties m n`` line: the protocol's baseline rows.  The protocol's baseline is computed on the
TRAIN graph (``--input train.npz``, what ``--task split`` wrote), not on the original, whose edges include the answers.
``--task fit`` trains an exact logistic regression on the GPU (``classify.fit``) and writes the model to ``--output``: with
``--pairs POS --neg_pairs NEG --operator {average,hadamard,l1,l2} [--l2_penalty X]`` the link classifier of the node2vec paper on
the vectors of the embedding file ``--input`` -- label 1 for the pairs of ``--pairs``, 0 for those of ``--neg_pairs``, positives
first; with ``--labels FILE`` (lines ``node<delimiter>0|1``) a node classifier on the rows themselves (operator ``row``).
``--task score --model model.tsv`` writes the model's decision value of every pair instead of the metric (and, with
``--neg_pairs``, the AUC of the decision values).  ``--operator``, ``--l2_penalty`` and ``--labels`` with another task, ``--model``
with a task other than ``score``, ``--metric`` beside ``--model`` and ``--operator`` beside ``--labels`` are ignored with a warning.
The sparse modes parse an ``.edg`` input on the GPU (``read_edg_device``); ``PECANPY_AMD_HOST_READER=1`` keeps the host reader.

    pecanpy --input demo/karate.edg --output karate.emb --mode SparseOTF --p 0.5 --q 2
"""
import argparse
import os
import warnings

import numpy as np

from . import graph
from . import pecanpy
from .wrappers import Timer

MODES = ("DenseOTF", "FirstOrderUnweighted", "PreComp", "PreCompFirstOrder", "SparseOTF")
HEURISTICS = ("common_neighbours", "jaccard", "adamic_adar", "resource_allocation", "preferential_attachment")   # --task baseline
OPERATORS = ("average", "hadamard", "l1", "l2")   # --task fit with pairs

# (flag, argparse keywords) -- one table instead of twenty add_argument calls
_OPTIONS = (
    ("--input", dict(required=True, help="graph file: .edg edge list or .npz (CSR / dense)")),
    ("--output", dict(default=None, help="embedding file (.npz -> IDs/data arrays, else word2vec text); required by every task but "
                                         "baseline")),
    ("--task", dict(default="pecanpy", choices=("pecanpy", "tocsr", "todense", "walks", "train", "neighbours", "score", "split", "baseline", "fit"),
                    help="run node2vec; only convert the edge list to CSR / dense .npz; (walks) generate the walks and "
                         "write them, one per line, to --output, no training; (train) train embeddings from a walk "
                         "corpus file given as --input, no graph; or (neighbours) the nearest neighbours of the nodes of an "
                         "embedding file given as --input, no graph; or (score) the score of every node pair of --pairs by an "
                         "embedding file given as --input, no graph; or (split) hold out --holdout_fraction of the edges of the "
                         "graph: the train graph as a CSR .npz to --output, the held-out pairs to --pairs; or (baseline) the "
                         "score of every node pair of --pairs by the neighbourhood heuristic --heuristic of the graph given as "
                         "--input (a sparse --mode), written to --output when given.  The link-prediction protocol computes its "
                         "baseline on the TRAIN graph (--input train.npz from --task split), not on the original graph, whose "
                         "edges include the answers; or (fit) train a logistic regression on the vectors of an embedding file given as "
                         "--input -- on --operator of the pairs of --pairs (label 1) and --neg_pairs (label 0), or on the rows of "
                         "the nodes of --labels -- and write the model to --output")),
    ("--mode", dict(default="SparseOTF", choices=MODES, help="walk engine variant")),
    ("--dimensions", dict(type=int, default=128, help="embedding size")),
    ("--walk-length", dict(type=int, default=80, help="steps per walk")),
    ("--num-walks", dict(type=int, default=10, help="walks per start vertex")),
    ("--window-size", dict(type=int, default=10, help="skip-gram window")),
    ("--epochs", dict(type=int, default=1, help="skip-gram epochs")),
    ("--workers", dict(type=int, default=0, help="host threads for the skip-gram stage (0 = all)")),
    ("--p", dict(type=float, default=1, help="return parameter")),
    ("--q", dict(type=float, default=1, help="in-out parameter")),
    ("--weighted", dict(action="store_true", help="third column of the edge list holds weights")),
    ("--directed", dict(action="store_true", help="do not add the reverse of every edge")),
    ("--verbose", dict(action="store_true", help="progress output")),
    ("--extend", dict(action="store_true", help="node2vec+ (weighted graphs)")),
    ("--gamma", dict(type=float, default=0, help="node2vec+ noisy-edge threshold = mean + gamma * std")),
    ("--random_state", dict(type=int, default=None, help="seed of the walk stream")),
    ("--epoch_loss", dict(action="store_true", help="GPU trainer only: print the skip-gram loss of every epoch (sum and mean "
                                                    "per evaluation); --workers 1 then also makes the trainer deterministic")),
    ("--fresh_walks", dict(action="store_true", help="GPU trainer only: every epoch after the first trains on newly drawn walks "
                                                     "(call seed random_state + epoch); implies the route of --epoch_loss")),
    ("--holdout_walks", dict(type=int, default=0, help="GPU trainer only: draw this many held-out walks per node once and print "
                                                       "their mean loss after every epoch; implies the route of --epoch_loss")),
    ("--init_emb", dict(default=None, metavar="FILE",
                        help="GPU trainer only: embed new nodes into old vectors -- an .npz with IDs / data as this program writes "
                             "it, or a word2vec text file; its nodes start from these vectors, the others from the seeded "
                             "initialisation; implies the route of --epoch_loss")),
    ("--freeze_init", dict(action="store_true", help="with --init_emb: the given vectors stay exactly as they are, only the other "
                                                     "nodes are trained")),
    ("--walks_from", dict(default="new", choices=("new", "all"),
                          help="with --init_emb: walks start from the nodes the file does not have (new) or from every node (all)")),
    ("--topn", dict(type=int, default=10, help="--task neighbours: neighbours per query")),
    ("--metric", dict(default="cosine", choices=("cosine", "dot"), help="--task neighbours / score: the score")),
    ("--queries", dict(default=None, metavar="FILE", help="--task neighbours: one node ID per line (default: every node)")),
    ("--pairs", dict(default=None, metavar="FILE", help="--task score / baseline: two node IDs per line, separated by --delimiter; "
                                                        "--task split: receives the held-out pairs in that form")),
    ("--neg_pairs", dict(default=None, metavar="FILE",
                         help="--task score / baseline: negative pairs in the same form; prints 'auc wins ties m n' of --pairs "
                              "against them; "
                              "--task split: receives as many non-edges of the original graph as there are held-out pairs")),
    ("--heuristic", dict(default=None, choices=HEURISTICS, metavar="KIND",
                         help="--task baseline: the neighbourhood heuristic, one of " + ", ".join(HEURISTICS))),
    ("--operator", dict(default="hadamard", choices=OPERATORS, help="--task fit with pairs: the binary operator on the two vectors")),
    ("--l2_penalty", dict(type=float, default=1e-3, help="--task fit: the weight of |w|^2 / 2 beside the mean log-loss")),
    ("--labels", dict(default=None, metavar="FILE", help="--task fit: one 'node<delimiter>0|1' line per labelled node (operator row)")),
    ("--model", dict(default=None, metavar="FILE", help="--task score: a model file of --task fit; the score is its decision value")),
    ("--holdout_fraction", dict(type=float, default=0.5, help="--task split: the share of the edges to hold out, in [0, 1)")),
    ("--no_protect", dict(action="store_true", help="--task split: do not keep the first edge of every node in the train graph")),
    ("--delimiter", dict(type=str, default="\t", help="column separator of the edge list")),
    ("--implicit_ids", dict(action="store_true", help=".npz without IDs: use 0..N-1")),
)


def parse_args(argv=None):
    """The reference's flag set (``--walk-length`` style and ``--random_state`` style both as there)."""
    parser = argparse.ArgumentParser(
        prog="pecanpy",
        description="node2vec / node2vec+ embeddings; random walks generated on AMD MI355X GPUs",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    for flag, kw in _OPTIONS:
        parser.add_argument(flag, **kw)
    args = parser.parse_args(argv)
    if args.task != "baseline" and args.output is None:
        parser.error("the following arguments are required: --output")
    if args.task in ("score", "split", "baseline") and not args.pairs:
        parser.error(f"--task {args.task} needs --pairs")
    fit_flags = [f for f, given in (("--operator", args.operator != parser.get_default("operator")), ("--labels", bool(args.labels)),
                                    ("--l2_penalty", args.l2_penalty != parser.get_default("l2_penalty"))) if given]
    if args.task != "fit" and fit_flags:
        warnings.warn(f"{', '.join(fit_flags)} belong to --task fit; --task {args.task} ignores them", stacklevel=2)
    if args.task == "fit" and args.labels and "--operator" in fit_flags:
        warnings.warn("--task fit with --labels trains on the rows themselves (operator row); --operator is ignored", stacklevel=2)
    if args.model and args.task != "score":
        warnings.warn(f"--model belongs to --task score; --task {args.task} ignores it", stacklevel=2)
    if args.model and args.task == "score" and args.metric != parser.get_default("metric"):
        warnings.warn("--task score with --model writes the model's decision value; --metric is ignored", stacklevel=2)
    if args.task == "fit":
        if bool(args.labels) == bool(args.pairs or args.neg_pairs) or (not args.labels and not (args.pairs and args.neg_pairs)):
            parser.error("--task fit needs either --labels, or --pairs together with --neg_pairs (and --operator)")
    if args.task == "baseline":
        if not args.heuristic:
            parser.error("--task baseline needs --heuristic")
        if args.mode == "DenseOTF":
            parser.error("--task baseline needs a sparse --mode, not DenseOTF")
        if not args.output and not args.neg_pairs:
            parser.error("--task baseline needs --output, --neg_pairs or both: there is nothing to write otherwise")
    return args


def _advise(better, current, why):
    warnings.warn(f"{why}: {better} is recommended over {current} (current selection)", stacklevel=3)


def check_mode(g, args):
    """Reject impossible mode / parameter combinations and recommend a better mode (cli.py:179-254)."""
    mode = args.mode
    first_order = args.p == 1 and args.q == 1

    # hard constraints of the two first-order modes
    if mode == "FirstOrderUnweighted" and (args.weighted or not first_order):
        raise ValueError(f"FirstOrderUnweighted only works when weighted = False and p = q = 1, got "
                         f"weighted={args.weighted}, p={args.p}, q={args.q}")
    if mode == "PreCompFirstOrder" and not first_order:
        raise ValueError(f"PreCompFirstOrder only works when p = q = 1, got p={args.p}, q={args.q}")
    if mode == "FirstOrderUnweighted":
        return

    # p = q = 1: a first-order mode does the same walk for less
    if first_order:
        if not args.weighted:
            _advise("FirstOrderUnweighted", mode, "p = q = 1 on an unweighted graph")
        elif mode != "PreCompFirstOrder":
            _advise("PreCompFirstOrder", mode, "p = q = 1")
        return

    # second order: pick by size and density
    n, rho = g.num_nodes, g.density
    if rho >= 0.2:
        best, why = "DenseOTF", f"network density = {rho:.3f} (>= 0.2)"
    elif rho < 0.001 and n < 10000:
        best, why = "PreComp", f"network density = {rho:.2e} (< 0.001) with {n} nodes (< 10000)"
    else:
        best, why = "SparseOTF", f"network density = {rho:.3g} with {n} nodes"
    if mode != best:
        _advise(best, mode, why)


def _convert_only(args):
    target = graph.SparseGraph() if args.task == "tocsr" else graph.DenseGraph()
    target.read_edg(args.input, args.weighted, args.directed, args.delimiter)
    target.save(args.output)
    raise SystemExit(0)


@Timer("load Graph")
def read_graph(args):
    """Build the graph object of ``--mode`` from ``--input`` (or convert and exit for tocsr/todense)."""
    if args.directed and args.extend:
        raise NotImplementedError("Node2vec+ not implemented for directed graph yet.")
    if args.extend and not args.weighted:
        print("NOTE: node2vec+ is equivalent to node2vec for unweighted graphs.")
    if args.task in ("tocsr", "todense"):
        _convert_only(args)

    engine_cls = getattr(pecanpy, args.mode)
    g = engine_cls(args.p, args.q, args.workers, args.verbose, args.extend, args.gamma, args.random_state)
    if args.input.endswith(".npz"):
        g.read_npz(args.input, args.weighted, implicit_ids=args.implicit_ids)
    elif hasattr(g, "read_edg_device") and not os.environ.get("PECANPY_AMD_HOST_READER"):
        # the edge list is parsed on the device, for the dense modes into the dense handle without an N x N host matrix (same
        # arrays, warnings and exceptions: read_edg_device falls back to read_edg by itself); PECANPY_AMD_HOST_READER=1 keeps
        # the host reader
        g.read_edg_device(args.input, args.weighted, args.directed, args.delimiter)
        if args.verbose:
            print(f"edge list read by the {g.last_build_stats['reader']} reader")
    else:
        g.read_edg(args.input, args.weighted, args.directed, args.delimiter)
    check_mode(g, args)
    return g


@Timer("pre-compute transition probabilities")
def preprocess(g):
    g.preprocess_transition_probs()


@Timer("generate walks")
def simulate_walks(args, g):
    return g.simulate_walks(args.num_walks, args.walk_length)


def _dump_walks(path, walks):
    with open(path, "w", encoding="utf-8") as out:
        out.writelines(" ".join(w) + "\n" for w in walks)


def _walk_matrix(g, walks):
    """ID lists -> uint32[n_walks, L + 2] (the engine's matrix; only needed when gensim is absent)."""
    index = {name: i for i, name in enumerate(g.nodes)}
    width = max((len(w) for w in walks), default=1) + 1
    mat = np.zeros((len(walks), width), dtype=np.uint32)
    for r, w in enumerate(walks):
        mat[r, : len(w)] = [index[x] for x in w]
        mat[r, -1] = len(w)
    return mat


@Timer("train embeddings")
def learn_embeddings(args, walks, g=None):
    """Skip-gram over the walk corpus (cli.py:307-325): gensim when it is installed, else the GPU trainer of this
    package (``pecanpy_amd.embed``); ``PECANPY_AMD_DUMP_WALKS=1`` writes the walks (one per line) instead."""
    if os.environ.get("PECANPY_AMD_DUMP_WALKS"):
        _dump_walks(args.output, walks)
        return
    try:
        from gensim.models import Word2Vec
    except ImportError:
        Word2Vec = None
    if Word2Vec is None:
        if g is None:
            _dump_walks(args.output, walks)
            warnings.warn(f"gensim is not installed and no graph was passed: {len(walks)} walks written to "
                          f"{args.output} instead of embeddings", stacklevel=2)
            return
        from .embed import train_sgns

        vecs = train_sgns(_walk_matrix(g, walks), g.num_nodes, dim=args.dimensions, window=args.window_size,
                          epochs=args.epochs, seed=args.random_state)
        _save_vectors(args, g, vecs)
        return
    w2v = Word2Vec(walks, vector_size=args.dimensions, window=args.window_size, min_count=0, sg=1,
                   workers=args.workers, epochs=args.epochs, seed=args.random_state)
    vectors = w2v.wv
    if args.output.endswith(".npz"):
        np.savez(args.output, IDs=vectors.index_to_key, data=vectors.vectors)
    else:
        vectors.save_word2vec_format(args.output)


def _gpu_route():
    """Graph -> vectors without ID lists: taken when gensim is absent and the walks are not asked for as text."""
    if os.environ.get("PECANPY_AMD_DUMP_WALKS"):
        return False
    try:
        import gensim  # noqa: F401
    except ImportError:
        return True
    return False


def _save_vectors(args, g, vecs):
    if args.output.endswith(".npz"):
        np.savez(args.output, IDs=g.nodes, data=vecs)
    else:
        from .embed import save_word2vec_format

        save_word2vec_format(args.output, g.nodes, vecs)


@Timer("generate walks + write them")
def walks_to_file(args, g):
    """``--task walks``: the walk corpus as text (``Base.walks_to_file``: formatted in device memory, no ID lists)."""
    g.walks_to_file(args.output, args.num_walks, args.walk_length)


@Timer("generate walks + train embeddings")
def embed_on_gpu(args, g):
    """Walks and skip-gram in device memory (``Base.embed_array``), the vectors written as ``learn_embeddings`` writes
    them; no ``List[List[str]]`` corpus and no index matrix on the host."""
    if args.init_emb:
        known_ids, vectors = _known_vectors(g, *read_init_emb(args.init_emb))
        with g.extend_session(known_ids, vectors, starts=args.walks_from, freeze=args.freeze_init, num_walks=args.num_walks,
                              walk_length=args.walk_length, window_size=args.window_size, epochs=args.epochs,
                              workers=_session_workers(args), compute_loss=True, fresh_walks=args.fresh_walks,
                              holdout_walks=args.holdout_walks) as session:
            _print_epoch_loss(session.run(args.epochs))
            vecs = session.vectors().cpu().numpy()
    elif args.epoch_loss or args.fresh_walks or args.holdout_walks:
        with g.embed_session(dim=args.dimensions, num_walks=args.num_walks, walk_length=args.walk_length,
                             window_size=args.window_size, epochs=args.epochs, workers=_session_workers(args),
                             compute_loss=True, fresh_walks=args.fresh_walks, holdout_walks=args.holdout_walks) as session:
            _print_epoch_loss(session.run(args.epochs))
            vecs = session.vectors().cpu().numpy()
    else:
        vecs = g.embed_array(dim=args.dimensions, num_walks=args.num_walks, walk_length=args.walk_length,
                             window_size=args.window_size, epochs=args.epochs)
    _save_vectors(args, g, vecs)


def read_init_emb(path):
    """``(ids, float32[n, dim])`` of an embedding file: an ``.npz`` with ``IDs`` / ``data`` as this program writes it, or a
    word2vec text file (a header line ``count dim``, then a name and ``dim`` numbers per line).  Read on the host."""
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            ids, data = [str(i) for i in z["IDs"].tolist()], np.ascontiguousarray(z["data"], dtype=np.float32)
    else:
        with open(path, encoding="utf-8") as f:
            count, dim = (int(x) for x in f.readline().split())
            rows = [line.rstrip("\n").split(" ") for line in f if line.strip()]
        if len(rows) != count or any(len(r) != dim + 1 for r in rows):
            raise ValueError(f"{path}: the header announces {count} rows of {dim} numbers, the file holds something else")
        ids = [r[0] for r in rows]
        data = np.array([r[1:] for r in rows], dtype=np.float32).reshape(count, dim)
    if data.ndim != 2 or data.shape[0] != len(ids):
        raise ValueError(f"{path}: {len(ids)} IDs for a data array of shape {list(data.shape)}")
    return ids, data


def _known_vectors(g, ids, data):
    """The rows of an ``--init_emb`` file that name a node of the graph; the others are dropped with one warning."""
    have = set(g.nodes)
    keep = [i for i, name in enumerate(ids) if name in have]
    if len(keep) != len(ids):
        warnings.warn(f"--init_emb: {len(ids) - len(keep)} of {len(ids)} IDs are not in the graph and are dropped", stacklevel=3)
    return [ids[i] for i in keep], np.ascontiguousarray(data[keep])


def _warn_init_flags_ignored(args, why):
    if args.init_emb or args.freeze_init:
        warnings.warn(f"--init_emb, --freeze_init and --walks_from belong to the GPU trainer on a graph; {why}", stacklevel=3)


def _warn_graph_flags_ignored(args, task):
    """The warnings of a task that has no graph (``train``, ``neighbours``) for the flags that need one."""
    if args.fresh_walks or args.holdout_walks:
        warnings.warn(f"--fresh_walks and --holdout_walks draw walks from a graph; --task {task} has none, so they are ignored",
                      stacklevel=3)
    _warn_init_flags_ignored(args, f"--task {task} has no graph, so they are ignored")


def _session_workers(args):
    """``--epoch_loss`` forwards ``--workers 1`` to the GPU trainer (one wavefront, deterministic); any other value keeps the
    trainer's default."""
    return 1 if args.cli_workers == 1 else 0


def _print_epoch_loss(records):
    for i, r in enumerate(records, 1):
        mean = r["loss"] / r["evaluations"] if r["evaluations"] else 0.0
        held = ""
        if "holdout_loss" in r:
            n = r["holdout_evaluations"]
            held = f", held-out mean {r['holdout_loss'] / n if n else 0.0:.6f} over {n} evaluations"
        print(f"epoch {i}: loss {r['loss']:.6f}, mean {mean:.6f} over {r['evaluations']} evaluations{held}")


@Timer("read corpus + train embeddings")
def train_from_corpus(args):
    """``--task train``: ``--input`` is a walk corpus file (what ``--task walks`` writes); it is read and numbered in device
    memory and trained there (``embed.train_sgns_file``); the vectors are written in order of first appearance."""
    from .embed import save_word2vec_format_device, sgns_session_file, train_sgns_file

    _warn_graph_flags_ignored(args, "train")

    if args.epoch_loss:
        names, session = sgns_session_file(args.input, dim=args.dimensions, window=args.window_size, epochs=args.epochs,
                                           seed=args.random_state, workers=_session_workers(args), compute_loss=True)
        with session:
            _print_epoch_loss(session.run(args.epochs))
            d_vectors = session.vectors()
    else:
        names, d_vectors = train_sgns_file(args.input, dim=args.dimensions, window=args.window_size, epochs=args.epochs,
                                           seed=args.random_state)
        if args.verbose:
            print(f"corpus read by the {train_sgns_file.last_stats['read']['reader']} reader")
    if args.output.endswith(".npz"):
        np.savez(args.output, IDs=names, data=d_vectors.cpu().numpy())
    else:
        save_word2vec_format_device(args.output, names, d_vectors)


@Timer("read embedding + nearest neighbours")
def neighbours_from_file(args):
    """``--task neighbours``: ``--input`` is an embedding file (``read_init_emb``: ``.npz`` with ``IDs`` / ``data``, or word2vec
    text); ``--output`` gets one line ``query<TAB>neighbour<TAB>%.6f`` per result, the queries in the order given (``--queries``:
    one ID per line; default every row), the neighbours in rank order (``embed.KnnIndex``: exact, ties by row number)."""
    from . import embed

    _warn_graph_flags_ignored(args, "neighbours")
    ids, data = read_init_emb(args.input)
    if args.queries:
        row_of = {name: i for i, name in enumerate(ids)}
        with open(args.queries, encoding="utf-8") as f:
            asked = [line.strip() for line in f if line.strip()]
        for name in asked:
            if name not in row_of:
                raise ValueError(f"{args.queries}: unknown node ID {name!r}")
        rows = np.array([row_of[name] for name in asked], dtype=np.int64)
    else:
        rows = np.arange(len(ids), dtype=np.int64)
    with embed.KnnIndex(data, node_ids=ids) as index:
        idx, score = index.query(rows=rows, topn=args.topn, metric=args.metric)
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    with open(args.output, "w", encoding="utf-8", newline="\n") as f:
        for r, ri, rs in zip(rows, idx, score):
            f.write("".join("%s\t%s\t%.6f\n" % (ids[r], ids[i], s) for i, s in zip(ri, rs) if i >= 0))


def _read_pairs(path, delimiter, row_of):
    """``(names_u, names_v, rows_u, rows_v)`` of a pair file: two node IDs per line, separated by ``delimiter``; an unknown ID
    or another number of fields is a ``ValueError`` naming the line."""
    nu, nv = [], []
    with open(path, encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            terms = line.split(delimiter)
            if len(terms) != 2:
                raise ValueError(f"{path}, line {no}: expected two node IDs, found {len(terms)} fields")
            for name in terms:
                if name not in row_of:
                    raise ValueError(f"{path}, line {no}: unknown node ID {name!r}")
            nu.append(terms[0])
            nv.append(terms[1])
    rows = [np.array([row_of[x] for x in names], dtype=np.int64) for names in (nu, nv)]
    return nu, nv, rows[0], rows[1]


@Timer("read embedding + score pairs")
def score_from_file(args):
    """``--task score``: ``--input`` is an embedding file (``read_init_emb``), ``--pairs`` a file of node pairs; ``--output`` gets
    one line ``id_u<delimiter>id_v<delimiter>score`` per pair, the score as ``repr(float)`` (``KnnIndex.score_pairs``: exact).  With
    ``--neg_pairs`` the line ``auc wins ties m n`` of the pairs' scores against those pairs' scores goes to stdout
    (``linkpred.auc``: exact integers, one rounding)."""
    from . import classify, embed, linkpred

    _warn_graph_flags_ignored(args, "score")
    ids, data = read_init_emb(args.input)
    row_of = {name: i for i, name in enumerate(ids)}
    nu, nv, ru, rv = _read_pairs(args.pairs, args.delimiter, row_of)
    neg = _read_pairs(args.neg_pairs, args.delimiter, row_of) if args.neg_pairs else None
    with embed.KnnIndex(data, node_ids=ids) as index:
        if args.model:   # the decision value of a fitted model instead of the metric
            model = classify.LogisticModel.load(args.model)
            d_pos = model.decision_function(index, ru, rv)
            d_neg = model.decision_function(index, neg[2], neg[3]) if neg else None
        else:
            d_pos = index.score_pairs(ru, rv, metric=args.metric)
            d_neg = index.score_pairs(neg[2], neg[3], metric=args.metric) if neg else None
        result = linkpred.auc(d_pos, d_neg) if neg else None
    d = args.delimiter
    with open(args.output, "w", encoding="utf-8", newline="\n") as f:
        f.write("".join(f"{a}{d}{b}{d}{float(s)!r}\n" for a, b, s in zip(nu, nv, d_pos.cpu().numpy())))
    if result:
        print(f"{result[0]!r} {result[1]} {result[2]} {len(nu)} {len(neg[0])}")


def _read_labels(path, delimiter, row_of):
    """``(rows, labels)`` of a label file: ``node<delimiter>0|1`` per line; anything else is a ``ValueError`` naming the line."""
    rows, labels = [], []
    with open(path, encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            terms = line.split(delimiter)
            if len(terms) != 2 or terms[1] not in ("0", "1"):
                raise ValueError(f"{path}, line {no}: expected a node ID and a label 0 or 1")
            if terms[0] not in row_of:
                raise ValueError(f"{path}, line {no}: unknown node ID {terms[0]!r}")
            rows.append(row_of[terms[0]])
            labels.append(int(terms[1]))
    return np.array(rows, dtype=np.int64), np.array(labels, dtype=np.uint8)


@Timer("read embedding + fit a logistic regression")
def fit_from_file(args):
    """``--task fit``: ``--input`` is an embedding file (``read_init_emb``).  With ``--pairs`` and ``--neg_pairs``: ``classify.fit``
    on ``--operator`` of the pairs, label 1 for ``--pairs`` and 0 for ``--neg_pairs``, positives first; with ``--labels``: on the
    rows of the labelled nodes (operator ``row``).  ``--output`` gets the model (``LogisticModel.save``); stdout the line
    ``loss n_iter n_eval converged``."""
    from . import classify, embed

    _warn_graph_flags_ignored(args, "fit")
    ids, data = read_init_emb(args.input)
    row_of = {name: i for i, name in enumerate(ids)}
    with embed.KnnIndex(data, node_ids=ids) as index:
        if args.labels:
            rows, y = _read_labels(args.labels, args.delimiter, row_of)
            model = classify.fit(index, rows, None, y, "row", l2=args.l2_penalty)
        else:
            pos, neg = _read_pairs(args.pairs, args.delimiter, row_of), _read_pairs(args.neg_pairs, args.delimiter, row_of)
            y = np.concatenate([np.ones(len(pos[0]), dtype=np.uint8), np.zeros(len(neg[0]), dtype=np.uint8)])
            model = classify.fit(index, np.concatenate([pos[2], neg[2]]), np.concatenate([pos[3], neg[3]]), y, args.operator, l2=args.l2_penalty)
    model.save(args.output)
    print(f"{model.loss!r} {model.n_iter} {model.n_eval} {int(model.converged)}")


def _write_pairs(path, delimiter, ids, u, v):
    with open(path, "w", encoding="utf-8", newline="\n") as f:
        f.write("".join(f"{ids[a]}{delimiter}{ids[b]}\n" for a, b in zip(u.cpu().tolist(), v.cpu().tolist())))


@Timer("hold out edges + write the train graph and the pairs")
def split_to_files(args, g):
    """``--task split``: ``Base.holdout_edges`` with ``--holdout_fraction``, the seed ``--random_state`` (0 when not given), each
    entry a unit with ``--directed``, no protection with ``--no_protect``.  ``--output`` gets the train graph as ``tocsr`` writes a
    CSR (``IDs`` / ``data`` / ``indptr`` / ``indices``), ``--pairs`` the held-out pairs as node IDs, one pair per line with
    ``--delimiter``, and ``--neg_pairs`` equally many non-edges of the ORIGINAL graph from the same seed
    (``Base.sample_non_edges``): what ``--task score`` reads."""
    seed = args.random_state or 0
    train, (u, v, _), _ = g.holdout_edges(args.holdout_fraction, seed, directed=args.directed, protect=not args.no_protect)
    train.save(args.output)
    _write_pairs(args.pairs, args.delimiter, g.nodes, u, v)
    if args.neg_pairs:
        nu, nv, _ = g.sample_non_edges(int(u.numel()), seed)
        _write_pairs(args.neg_pairs, args.delimiter, g.nodes, nu, nv)
    if args.verbose:
        print(f"held out {g.last_holdout_stats['held']} of {g.last_holdout_stats['units']} edges "
              f"({g.last_holdout_stats['protected']} protected)")


@Timer("score pairs by a neighbourhood heuristic")
def baseline_from_graph(args, g):
    """``--task baseline``: ``--input`` is a graph, read as ``--task split`` reads it (a sparse ``--mode``); in the link-prediction
    protocol it is the TRAIN graph that ``--task split`` wrote, not the original, whose edges include the answers.  ``--pairs`` is a
    file of node pairs, mapped to rows as ``--task score`` maps them; ``--output``, when given, gets one line
    ``id_u<delimiter>id_v<delimiter>score`` per pair, the score as ``repr(float)`` (``Base.neighbour_scores``: exact).  With
    ``--neg_pairs`` the line ``auc wins ties m n`` goes to stdout (``linkpred.auc``)."""
    from . import linkpred

    row_of = {name: i for i, name in enumerate(g.nodes)}
    nu, nv, ru, rv = _read_pairs(args.pairs, args.delimiter, row_of)
    neg = _read_pairs(args.neg_pairs, args.delimiter, row_of) if args.neg_pairs else None
    d_pos = g.neighbour_scores(ru, rv, args.heuristic)
    result = linkpred.auc(d_pos, g.neighbour_scores(neg[2], neg[3], args.heuristic)) if neg else None
    d = args.delimiter
    if args.output:
        with open(args.output, "w", encoding="utf-8", newline="\n") as f:
            f.write("".join(f"{a}{d}{b}{d}{float(s)!r}\n" for a, b, s in zip(nu, nv, d_pos.cpu().numpy())))
    if result:
        print(f"{result[0]!r} {result[1]} {result[2]} {len(nu)} {len(neg[0])}")


def main(argv=None):
    """read graph -> preprocess -> walks (GPU) -> embeddings; ``--task train``: corpus file -> embeddings; ``--task
    neighbours``: embedding file -> nearest neighbours."""
    args = parse_args(argv)
    args.cli_workers = args.workers   # (as given: below, 0 becomes the host's thread count for gensim)
    if args.task == "train":   # no graph: the graph flags are ignored
        train_from_corpus(args)
        return
    if args.task == "neighbours":
        neighbours_from_file(args)
        return
    if args.task == "score":
        score_from_file(args)
        return
    if args.task == "fit":
        fit_from_file(args)
        return
    args.workers = args.workers or (os.cpu_count() or 1)
    g = read_graph(args)
    if args.task == "split":
        split_to_files(args, g)
        return
    if args.task == "baseline":
        baseline_from_graph(args, g)
        return
    preprocess(g)
    if args.task == "walks":
        walks_to_file(args, g)
    elif _gpu_route():
        embed_on_gpu(args, g)
    else:
        if args.epoch_loss:
            warnings.warn("--epoch_loss reports the loss of the GPU trainer; gensim is importable (or the walks are dumped), "
                          "so that route runs as without the flag and no loss is printed", stacklevel=2)
        if args.fresh_walks or args.holdout_walks:
            warnings.warn("--fresh_walks and --holdout_walks belong to the GPU trainer; gensim is importable (or the walks are "
                          "dumped), so that route runs as without the flags", stacklevel=2)
        _warn_init_flags_ignored(args, "gensim is importable (or the walks are dumped), so that route runs as without the flags")
        learn_embeddings(args, simulate_walks(args, g), g)


if __name__ == "__main__":
    main()
