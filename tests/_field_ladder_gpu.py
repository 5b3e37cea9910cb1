"""The GPU side of the accuracy ladder (tests/_field_arithmetic.py): run one engine on one case and set its errors against the
bars.  Shared by tests/test_gpu_field_ladder.py and tools/field_accuracy_report.py."""
import copy
import importlib

import _field_arithmetic as A

DEV = "cuda"
_NETS = {}


def device_net(case):
    key = case.input_key
    if key not in _NETS:
        _NETS[key] = copy.deepcopy(A.inputs_of(case)["net"]).to(DEV).eval()
    return _NETS[key]


def run_engine(case, engine):
    """-> the engine's output for the case: the field [B, N, F + 4] or the render's (features, depth, weights)."""
    i, net = A.inputs_of(case), device_net(case)
    d = lambda t: t.to(DEV)
    if case.kind == "field":
        return net(d(i["pts"]), d(i["freq"]), d(i["phase"]), d(i["geo"]), d(i["dirs"]) if case.dirs else None, input_scaler=i["scaler"],
                   precision=engine)
    clamp, last_back, white_back = case.mode
    kw = dict(input_scaler=i["scaler"], noise=d(i["noise"]), clamp_mode=clamp, last_back=last_back, white_back=white_back, precision=engine)
    if case.kind == "render":
        return net.render(d(i["pts"]), d(i["freq"]), d(i["phase"]), d(i["geo"]), None, d(i["z"]), case.S, **kw)
    smpl = importlib.import_module("3dhumangan_amd.lib.components.smpl")
    c = {k: d(v) for k, v in i["cond"].items()}
    vik = smpl.vertex_inverse_transforms(c["fk_matrices"], c["lbs_weights"])
    idx = smpl.nearest_vertex(d(i["pts"]), c["vertices"])
    net.refine_last_sample = case.refine            # False: the engine alone; True: the shipped x2 render with its x3 relaunch
    return net.render_geo(d(i["pts"]), d(i["freq"]), d(i["phase"]), idx, c["skeletons_xyz"], c["vertices"], c["tpose_vertices"], vik, None,
                          d(i["z"]), case.S, **kw)


def measure(case, engine):
    """-> one record per (assertion, group): the engine's measured error, the bar, the healthy reference arithmetic's own figure,
    and whether the bar is asserted (Case.no_dist)."""
    L, ref = A.ladder_of(case), A.outputs_of(case)
    got = run_engine(case, engine)
    got = got.cpu() if case.kind == "field" else [t.cpu() for t in got]
    records = []
    for assertion, against in A.assertions_for(engine):
        err = A.errors(case, got, ref[against])
        for g in L["groups"]:
            bar = L["bars"][assertion][g]
            records.append(dict(case=case.name, engine=engine, assertion=assertion, against=against, group=g, measured=err[g], bar=bar,
                                healthy_reference=L["healthy"][assertion][g], headroom=bar / max(err[g], 1e-300),
                                asserted=A.asserted(case, assertion, g)))
    return records
