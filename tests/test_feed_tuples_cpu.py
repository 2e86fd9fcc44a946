"""CPU: the host tuples of FrameBatcher, CAVBatcher, M3AEBatcher and Modal3Batcher, byte for byte.  The digests in
tests/golden/feed_tuples_small.json were recorded by tests/golden/make_golden_feed_tuples.py (which documents the dataset, the
configurations and what is digested) with threads=1 and ring=4; the batches must not depend on either."""
import importlib.util
import json
import os

import pytest


@pytest.fixture(scope="module")
def gen(golden_dir):
    spec = importlib.util.spec_from_file_location("make_golden_feed_tuples", os.path.join(golden_dir, "make_golden_feed_tuples.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def dataset(gen, tmp_path_factory):
    return gen.build_dataset(str(tmp_path_factory.mktemp("feed_tuples")))


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "feed_tuples_small.json")) as f:
        return json.load(f)


def test_golden_covers_every_configuration(gen, golden):
    assert sorted(golden) == sorted(gen.CONFIGS) and len(golden) == 7
    for config, epochs in golden.items():
        assert len(epochs) == 2 and all(len(e) == 3 for e in epochs)
        assert all(sorted(b) == sorted(gen.CONFIGS[config][1]) for e in epochs for b in e)
        assert epochs[0] != epochs[1] or config.endswith("eval")           # set_epoch reseeds the draws of the train transforms


@pytest.mark.parametrize("ring", [2, 4])
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("config", ["frames_train", "frames_eval", "cav_train_augnois", "cav_eval", "m3ae_train", "m3ae_eval",
                                    "modal3_train"])
def test_host_tuples_equal_the_recorded_digests(gen, dataset, golden, config, threads, ring):
    names, paths = dataset
    got = gen.config_digests(config, names, paths, threads=threads, ring=ring)
    for e, (g_epoch, w_epoch) in enumerate(zip(got, golden[config])):
        for b, (g, w) in enumerate(zip(g_epoch, w_epoch)):
            differ = [k for k in w if g[k] != w[k]]
            assert not differ, f"{config}, epoch {e}, batch {b}: {differ} differ from the recorded bytes"
