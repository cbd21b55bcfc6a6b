"""The slot maps (_grad_slots) and plane tables (weight_table_with_planes) of PCTransformer, SconeOcc and SconeVis as each class spelled
them out itself before packing.table_slots / packing.planes_tail existed, restated as functions of the module: the frozen statement
tests/test_network_modules_cpu.py compares the shared helpers with."""
from macarons_amd.networks.packing import encoder_weight_planes, padded_weight_planes, weight_planes


def _encoder_slots(slots, encoders):
    for e, enc in enumerate(encoders):
        o = 4 + 12 * e
        qk = enc.mhsa.w_q.weight.shape[0]
        rows = ((0, qk), (qk, 2 * qk), (2 * qk, 2 * qk + enc.mhsa.w_v.weight.shape[0]))
        for lin, r in zip((enc.mhsa.w_q, enc.mhsa.w_k, enc.mhsa.w_v), rows):
            slots[id(lin.weight)], slots[id(lin.bias)] = (o + 2, r), (o + 3, r)
        for k, t in enumerate((enc.norm1.weight, enc.norm1.bias)):
            slots[id(t)] = (o + k, None)
        for k, t in enumerate((enc.mhsa.out.weight, enc.mhsa.out.bias, enc.norm2.weight, enc.norm2.bias, enc.ff.linear1.weight,
                               enc.ff.linear1.bias, enc.ff.linear2.weight, enc.ff.linear2.bias)):
            slots[id(t)] = (o + 4 + k, None)


def _finish(m, slots, name):
    params = tuple(m.parameters())
    missing = [n for n, p in m.named_parameters() if id(p) not in slots]
    if missing:
        raise NotImplementedError(f"{name} HIP backward: parameters outside the weight table: {missing}")
    return params, tuple(slots[id(p)] for p in params)


def pct_grad_slots(m):
    slots = {id(t): (k, None) for k, t in enumerate((m.embedding.linear1.weight, m.embedding.linear1.bias,
                                                      m.embedding.linear2.weight, m.embedding.linear2.bias))}
    _encoder_slots(slots, m.encoders)
    for k, t in enumerate((m.norm.weight, m.norm.bias, m.linear0.weight, m.linear0.bias)):
        slots[id(t)] = (28 + k, None)
    return _finish(m, slots, "PCTransformer")


def vis_grad_slots(m):
    slots = {id(m.embedding.linear1.weight): (0, None), id(m.embedding.linear1.bias): (1, None),
             id(m.embedding.linear2.weight): (2, None), id(m.embedding.linear2.bias): (3, None)}
    _encoder_slots(slots, m.encoders)
    for k, t in enumerate((m.norm.weight, m.norm.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.fc3.weight, m.fc3.bias)):
        slots[id(t)] = (40 + k, None)
    return _finish(m, slots, "SconeVis")


def occ_grad_slots(m):
    slots, o = {}, 0
    for t in (m.global_transformer, *m.local_transformers):
        ps, sl = pct_grad_slots(t)
        for p_, (k, rows) in zip(ps, sl):
            slots[id(p_)] = (o + k, rows)
        o += len(t.weight_table())
    for lin in (m.x_embedding.linear1, m.x_embedding.linear2, m.x_embedding.linear3, m.linear1, m.linear2, m.linear3):
        slots[id(lin.weight)], slots[id(lin.bias)] = (o, None), (o + 1, None)
        o += 2
    return _finish(m, slots, "SconeOcc")


def pct_planes(m):
    t = m.weight_table()
    for e in m.encoders:
        t += encoder_weight_planes(e)
    t += list(padded_weight_planes(m.embedding.linear2.weight, m.embedding.linear2.bias, 128, 128))
    t += [weight_planes(m.linear0.weight)]
    return t


def vis_planes(m):
    t = m.weight_table()
    for e in m.encoders:
        t += encoder_weight_planes(e)
    t += list(padded_weight_planes(m.embedding.linear2.weight, m.embedding.linear2.bias, 128, 128))
    t += [weight_planes(m.fc1.weight), weight_planes(m.fc2.weight), weight_planes(m.fc3.weight)]
    return t


def occ_planes(m):
    t = m.weight_table()
    g = m.global_transformer
    for e in g.encoders:
        t += encoder_weight_planes(e)
    t += list(padded_weight_planes(g.embedding.linear2.weight, g.embedding.linear2.bias, 128, 128))
    t += [weight_planes(g.linear0.weight)]
    return t
