"""The box-loss mode matrix of tests/golden/boxloss.npz (make_boxloss_golden.py) and tests/test_*_boxloss.py.

A mode is (name, spec).  spec keys: ``wise`` (WiseIouLoss, reference utils/metrics.py:567, or the bbox_iou family, :75-538),
``ltype`` (the WiseIouLoss ltype / the bbox_iou flag, 'MPDIoU' = bbox_*mpdiou), ``mono`` (Wise: None = v1, True = v2, False = v3),
``variant`` (None, 'inner', 'focaler'), ``nwd`` (BboxLoss.nwd_loss) and the keyword arguments that differ from the reference's
call-site values (``scale`` for ShapeIoU, ``d`` / ``u`` for Focaler).
"""
WISE_LTYPES = ("IoU", "WIoU", "EIoU", "GIoU", "DIoU", "CIoU", "SIoU", "ShapeIoU", "PIoU", "PIoU2", "MPDIoU")
BBOX_TYPES = ("IoU", "GIoU", "DIoU", "CIoU", "EIoU", "SIoU", "ShapeIoU", "PIoU", "PIoU2", "MPDIoU")
VARIANTS = (None, "inner", "focaler")
FM = {None: "v1", True: "v2", False: "v3"}


def _name(s):
    n = ("w_" if s["wise"] else "b_") + s["ltype"]
    if s["wise"]:
        n += "_" + FM[s["mono"]]
    n += "_" + (s["variant"] or "plain")
    if "scale" in s:
        n += f"_s{s['scale']}"
    if "d" in s:
        n += f"_d{s['d']}u{s['u']}"
    if s["nwd"]:
        n += "_nwd"
    return n


def _spec(wise, ltype, variant=None, mono=False, nwd=False, **kw):
    return dict(wise=wise, ltype=ltype, mono=mono if wise else None, variant=variant, nwd=nwd, **kw)


def boxloss_modes():
    specs = [_spec(True, lt, v) for lt in WISE_LTYPES for v in VARIANTS]
    specs += [_spec(True, lt, None, mono) for lt in ("WIoU", "CIoU", "SIoU", "MPDIoU") for mono in (None, True)]
    specs += [_spec(False, t, v) for t in BBOX_TYPES for v in VARIANTS]
    specs += [_spec(True, "SIoU", "focaler", nwd=True), _spec(False, "GIoU", "focaler", nwd=True), _spec(False, "MPDIoU", "inner", nwd=True)]
    specs += [_spec(True, "ShapeIoU", None, scale=0.5), _spec(False, "CIoU", "focaler", d=0.05, u=0.9)]
    return {_name(s): s for s in specs}


# modes that also run on one_gt / ragged / no_gt (every mode runs on random5, overlap and tiny)
SUBSET = ("w_WIoU_v3_inner", "w_CIoU_v1_plain", "w_SIoU_v3_focaler", "w_MPDIoU_v2_plain", "w_PIoU2_v3_plain", "w_ShapeIoU_v3_inner",
          "b_IoU_plain", "b_SIoU_inner", "b_EIoU_focaler", "b_PIoU_plain", "b_MPDIoU_focaler", "b_GIoU_focaler_nwd")
FULL_CASES = ("random5", "overlap", "tiny")
SUBSET_CASES = ("one_gt", "ragged", "no_gt")
# StepPlan end to end (DEAL-YOLO-N, models.npz's batch)
STEP_MODES = ("w_SIoU_v3_focaler", "b_EIoU_inner", "w_MPDIoU_v2_plain_nwd")


def step_spec(name):
    if name == "w_MPDIoU_v2_plain_nwd":
        return _spec(True, "MPDIoU", None, True, nwd=True)
    return boxloss_modes()[name]


def cases_of(mode):
    return FULL_CASES + (SUBSET_CASES if mode in SUBSET else ())


def n_calls(spec, case):
    return 3 if (spec["wise"] and case == "random5") else 1


def apply_mode(bbox_loss, spec, WiseIouLoss):
    """Select ``spec`` on a BboxLoss of this package (the reference's is selected by make_boxloss_golden.py)."""
    bbox_loss.nwd_loss = spec["nwd"]
    bbox_loss.use_wiseiou = spec["wise"]
    if spec["wise"]:
        bbox_loss.wiou_loss = WiseIouLoss(spec["ltype"], spec["mono"], spec["variant"] == "inner", spec["variant"] == "focaler")
    else:
        bbox_loss.iou_type, bbox_loss.iou_variant = spec["ltype"], spec["variant"]
    bbox_loss.shape_scale = spec.get("scale", 0.0)
    bbox_loss.focaler_d, bbox_loss.focaler_u = spec.get("d", 0.0), spec.get("u", 0.95)
