"""The routes of the parsimony path and the hooks that select each (tests/test_gpu_pug.py runs every test through all of them,
tests/test_gpu_id_ceilings.py the top of the id spaces)."""

PUG_ROUTES = {
    "phase-kernels": {},
    "one-workgroup": {"AFQ_TEST_PUG_ROUTE": "mono"},
    "handed-back": {"AFQ_TEST_P2_PART_CAP": "24"},
    "cover-1024": {"AFQ_TEST_P2_BIG_READS": "300"},
    "graph-per-cell": {"AFQ_TEST_P2_GRAPH": "cell"},
    "graph-per-cell-1024": {"AFQ_TEST_P2_GRAPH": "cell", "AFQ_TEST_P2_BIG_READS": "300", "AFQ_TEST_P2_DEFER_MIN": "0"},
    "graph-per-cell-ties-set-aside": {"AFQ_TEST_P2_GRAPH": "cell", "AFQ_TEST_P2_DEFER_MIN": "0"},
}


def set_pug_route(monkeypatch, name):
    for k, v in PUG_ROUTES[name].items():
        monkeypatch.setenv(k, v)
    return name
