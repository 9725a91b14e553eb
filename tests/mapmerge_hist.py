"""CausalBase-shaped map histories split into two replicas -- shared by
test_map_merge_oracle.py (CPU) and test_gpu_map_merge.py (the mirror).

A history is a run of map nodes with Lamport ids: writes and hides under a key
(cause = the key) and undo / redo nodes whose id cause names a key-caused node,
which is the only shape CausalBase makes.  Each node goes to replica a, replica
b or both; an id-caused node only where its cause is, so both replicas are
causally closed, and their node dicts keep history order (no insert of a merge
in that order can throw)."""
import random

from oracle import causal_ref as R

KEYS = ["k0", "k1", "k2", "k3"]
UUID = "U" * R.UUID_LENGTH


def history(seed, n_max=40, n_sites=3, n_keys=4):
    """[(id, cause, value)] in history (causal) order, at most n_max nodes."""
    rng = random.Random(seed)
    sites = [R.new_site_id(rng) for _ in range(n_sites)]
    nodes, key_caused = [], []
    for m in range(rng.randint(1, n_max)):
        i = (m + 1, rng.choice(sites), 0)
        r = rng.random()
        if r < 0.6 or not key_caused:
            v = R.HIDE if rng.random() < 0.2 else rng.randint(0, 9)
            nodes.append((i, rng.choice(KEYS[:n_keys]), v))
            key_caused.append(i)
        else:
            nodes.append((i, rng.choice(key_caused), rng.choice([R.H_HIDE, R.H_SHOW, R.HIDE])))
    return nodes


def split(nodes, seed, overlap=0.3):
    """Two causally closed node dicts (history order kept) whose union is `nodes`."""
    rng = random.Random(seed)
    a, b = {}, {}
    for i, cause, v in nodes:
        where = [x for x in (a, b) if not R.valid_id(cause) or cause in x]
        if len(where) == 2 and rng.random() >= overlap:
            where = [rng.choice(where)]
        for x in where:
            x[i] = (cause, v)
    return a, b


def ref_ct(nodes, site="S" * R.SITE_ID_LENGTH):
    """The reference's map ct of a node dict (s/refresh-caches)."""
    ct = R.new_map_ct(site_id=site, uuid=UUID)
    ct["nodes"] = dict(nodes)
    return R.refresh_caches(R.map_weave, ct)
