"""CPU checks of tests/vocab_cases.py: the restated loader, descent and transform (tests/vocab_ref.py) agree with the
oracle on the hand-written vocabulary for every feature count and levelsup and for every scoring / weighting pair;
every census item is realised; each base feature's hand-written leaf, word and weight equal the reference's."""
import numpy as np
import pytest

import vocab_cases as vc
import vocab_ref as ref


@pytest.fixture(scope="module")
def voc(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("voc") / "planted.bin")
    vc.write(path)
    return path, ref.Vocabulary(path)


def _each(v, feats, levelsup):
    return [v.transform_one(f, levelsup) for f in feats]


@pytest.mark.parametrize("levelsup", sorted(vc.LEVELSUP.values()))
@pytest.mark.parametrize("n", vc.COUNTS)
def test_reference_equals_oracle(oracle_mod, voc, n, levelsup):
    path, v = voc
    ov = oracle_mod.OracleVocabulary(path)
    assert (ov.k, ov.L, ov.scoring, ov.weighting, ov.nnodes, ov.nwords) == (v.k, v.L, 0, 0, len(v.nodes), len(v.words))
    feats, _ = vc.features(n, seed=n)
    want = _each(v, feats, levelsup)
    ow, owt, ond = ov.transform_each(feats, levelsup)
    assert ow.tolist() == [w[0] for w in want]
    assert owt.tolist() == [w[1] for w in want]
    defined = [i for i, w in enumerate(want) if w[2] is not None]
    assert ond[defined].tolist() == [want[i][2] for i in defined]
    bow, fv = v.transform(feats, levelsup)
    obow, ofv = ov.transform(feats, levelsup)
    assert obow == bow and list(obow) == list(bow)
    if None not in fv:
        assert ofv == fv and list(ofv) == list(fv)


@pytest.mark.parametrize("scoring,weighting", vc.PAIRS)
def test_scoring_weighting_pairs_equal_oracle(oracle_mod, tmp_path, scoring, weighting):
    path = str(tmp_path / "v.bin")
    vc.write(path, scoring, weighting)
    v, ov = ref.Vocabulary(path), oracle_mod.OracleVocabulary(path)
    for names in (vc.ALL_STOPPED, vc.SHARED):
        feats, _ = vc.features(len(names) * 2, seed=7, names=names)
        bow, fv = v.transform(feats, 2)
        obow, ofv = ov.transform(feats, 2)
        assert obow == bow and ofv == fv, (names, bow, obow)
        if names is vc.ALL_STOPPED:
            assert bow == {} and fv == {}
        else:
            assert set(bow) == {0, 4, 7} and fv == {1: [0, 1, 4, 5], 8: [3, 7], 10: [2, 6]}


def test_census(voc):
    path, v = voc
    rec, d, names = vc.tree()
    seen = set()
    depth = {0: 0}
    for nid in range(1, len(v.nodes)):          # parents may come later: resolve by walking up
        chain, p = 0, nid
        while p != 0:
            p, chain = v.nodes[p].parent, chain + 1
        depth[nid] = chain
    leaves = [n for n in range(1, len(v.nodes)) if not v.nodes[n].children]
    assert {depth[n] for n in leaves} == {1, 2, 3} and max(depth.values()) == vc.L
    seen |= {"leaf_at_depth_1", "leaf_at_depth_L"}
    counts = {len(n.children) for n in v.nodes}
    assert {1, 2, vc.K} <= counts
    seen |= {"node_with_1_child", "node_with_2_children", "node_with_k_children"}
    assert [r[0] for r in rec][:5] == [0, 1, 2, 2, 2]             # a child right after its parent, before its uncles
    seen.add("records_depth_first")
    assert any(r[0] > i + 1 for i, r in enumerate(rec)) and v.nodes[9].parent == 10
    seen.add("parent_id_above_child")
    assert v.nodes[0].children == [1, 8, 10] and v.nodes[10].children == [9, 11, 12, 13]
    seen.add("children_not_contiguous")
    assert (v.nodes[9].descriptor == v.nodes[11].descriptor).all() and v.nodes[9].parent == v.nodes[11].parent
    seen.add("identical_sibling_descriptors")
    assert len(v.nodes) == len(rec) + 2 and (v.nodes[13].descriptor == v.nodes[12].descriptor).all()
    assert v.nodes[13].word_id == 8 and len(v.words) == 9 and v.nodes[13].parent == 10
    seen.add("eof_duplicate_record")
    base = vc.base_features()
    for name, (desc, node, word, weight) in base.items():
        for levelsup in vc.LEVELSUP.values():
            w, wt, nid, path_ = v.transform_one(desc, levelsup)
            assert (path_[-1][0], w, wt) == (node, word, weight), (name, levelsup)
            nid_level = vc.L - levelsup
            assert nid == (0 if nid_level <= 0 else path_[nid_level - 1][0] if nid_level <= len(path_) else None)
    assert v.transform_one(base["Ca"][0], 0)[3][-1][1:3] == (0, True)
    assert v.transform_one(base["Cc"][0], 0)[3][-1] == (12, 0, True, 4)
    seen.add("nearest_is_last_record")
    p = v.transform_one(base["A1a_A1b_tie"][0], 0)[3][-1]
    assert p == (3, 20, True, 3)
    seen.add("equal_distance_first_child_wins")
    assert base["A1b"][3] == 0.0
    seen.add("stopped_word")
    for n in vc.COUNTS:
        feats, who = vc.features(n, seed=n)
        assert len(feats) == n
        for item, levelsup in vc.LEVELSUP.items():
            res = _each(v, feats, levelsup)
            assert [(r[3][-1][0], r[0], r[1]) for r in res] == [base[nm][1:] for nm in who], (n, item)
            undefined = [r[2] is None for r in res]
            if item == "levelsup_0" and n > 1:
                assert any(undefined) and not all(undefined)
                seen.add("nid_uninitialised_reads_0")
            if item != "levelsup_0":
                assert not any(undefined)
            seen.add(item)
        seen.add(f"n_{n}")
    feats, _ = vc.features(6, seed=7, names=vc.ALL_STOPPED)
    assert all(r[1] == 0.0 for r in _each(v, feats, 2))
    seen.add("all_words_stopped")
    feats, _ = vc.features(8, seed=7, names=vc.SHARED)
    words = [r[0] for r in _each(v, feats, 2)]
    assert words.count(0) == 4
    seen.add("two_features_share_a_word")
    assert len(vc.PAIRS) == 24 and len(set(vc.PAIRS)) == 24
    seen.add("every_scoring_weighting_pair")
    assert seen == set(vc.ITEMS), set(vc.ITEMS) ^ seen
