"""The plan of one head's similarity term list -- how WSROIHead.get_similarity_matrices (the reference's modeling/roi_heads/roi_heads.py:245-336)
reads MODEL.ROI_HEADS.FINETUNE_TERMS.{CLASSIFIER,BBOX,MASK} under MODEL.ROI_HEADS.VISUAL_ATTENTION_HEAD.SIMILARITY_COMBINATION.

The reference's rules, kept as they are:
  * 'lingual', 'visual', 'Average' and 'None' are found by list membership (:271, :316, :318, :321);
  * 'TopK', 'WTopK', 'LSDA' and 'VisualK' are found as SUBSTRINGS of any entry (:273, :284, :295, :306), and a family's k is
    int(entry.split("-")[1]) of the FIRST entry that contains its name -- "WTopK-5" contains "TopK", so ['WTopK-5'] alone is the TopK
    term plus the WTopK term, both with k = 5, and ['WTopK-5', 'TopK-3'] gives TopK k = 5 too;
  * every term is weighted 1 / len(list) (:270), whatever the number of terms that the list switches on;
  * "Product" (:325-332) multiplies into a zero matrix and takes softmax of the result: 1 / n_base for every non-empty list.
What the reference cannot evaluate, or what it would silently ignore, is refused with `inference.UnsupportedConfig`."""
from typing import NamedTuple

FAMILIES = ("TopK", "WTopK", "LSDA", "VisualK")          # substring-matched, "-k" suffix
WORDS = ("lingual", "visual", "Average", "None")          # membership-matched
COMBINATIONS = ("Sum", "Product")

UNKNOWN_TERM = ("FINETUNE_TERMS entry {entry!r} is not a similarity term: the reference knows 'lingual', 'visual', 'Average', 'None' (whole "
                "entries) and 'TopK-k', 'WTopK-k', 'LSDA-k', 'VisualK-k' (roi_heads.py:271-321); it would count the entry in the 1 / len(terms) "
                "weight and add nothing for it")
BAD_K = ("FINETUNE_TERMS entry {entry!r}: k must be an integer in [1, {n_base}] (the number of base classes) written as '{family}-k' -- the "
         "reference takes int(entry.split('-')[1]) of the first entry that contains '{family}' and torch.topk raises outside that range "
         "(roi_heads.py:274-311)")
VISUAL_WITH_VISUALK = ("'visual' together with a 'VisualK' term in one FINETUNE_TERMS list is not supported: the reference adds an [R, 1, b] "
                       "term to the [R, n, b] matrix after another unsqueeze(0) and builds a 4-D tensor (roi_heads.py:315-317)")
VISUALK_WITH_REGRESSION_BRANCH = (
    "a 'VisualK' term in MODEL.ROI_HEADS.FINETUNE_TERMS together with WEAK_DETECTOR.REGRESSION_BRANCH is not supported: it reads "
    "evaluation(...)[0][0] as a list of refinement streams (roi_heads.py:308), which under the switch is one [R, K+1] tensor -- the same "
    "failure as a \"visual\" term's (roi_heads.py:250-252)")
BAD_COMBINATION = ("MODEL.ROI_HEADS.VISUAL_ATTENTION_HEAD.SIMILARITY_COMBINATION {combination!r} is not supported: 'Sum' (roi_heads.py:269-324) or "
                   "'Product' (the reference's else branch, :325-332, which any other value would silently take)")


class Plan(NamedTuple):
    """one head's term list, parsed. `weight` = 1 / len(terms) (0 for an empty list); a k of 0 = the term is absent"""
    n_terms: int
    weight: float
    lingual: bool
    visual: bool
    topk: int
    wtopk: int
    lsda: int
    visualk: int
    average: bool
    none: bool
    product: bool

    @property
    def plain(self):
        """exactly 'lingual' and / or 'visual' under "Sum" (or no term at all): unit_similarity / unit_similarity_bwd as before"""
        return (not self.product and not (self.topk or self.wtopk or self.lsda or self.visualk or self.average or self.none)
                and self.n_terms == int(self.lingual) + int(self.visual))

    @property
    def key(self):
        return (self.lingual, self.visual)

    @property
    def zero(self):
        """the matrix is zero: no term, or 'None' under "Sum" """
        return self.n_terms == 0 or (self.none and not self.product)

    @property
    def constant(self):
        """the matrix does not depend on the weights or the RoIs"""
        return self.zero or self.product or self.average

    @property
    def per_roi(self):
        """does the matrix depend on the RoI's refinement logits (and pass a gradient to them)?"""
        return not self.constant and (self.visual or self.visualk > 0)

    @property
    def static_key(self):
        """what unit_similarity_static computes for this plan"""
        return (self.weight, self.lingual, self.topk, self.wtopk, self.lsda)


def _unsupported(msg):
    from .inference import UnsupportedConfig
    return UnsupportedConfig(msg)


def _family_k(terms, family, n_base):
    hits = [x for x in terms if family in x]
    if not hits:
        return 0
    parts = hits[0].split("-")
    try:
        k = int(parts[1])
    except (IndexError, ValueError):
        raise _unsupported(BAD_K.format(entry=hits[0], family=family, n_base=n_base)) from None
    if not 1 <= k <= n_base:
        raise _unsupported(BAD_K.format(entry=hits[0], family=family, n_base=n_base))
    return k


def parse_terms(terms, combination, n_base):
    """terms: one head's FINETUNE_TERMS list; combination: SIMILARITY_COMBINATION; n_base: number of base classes -> Plan"""
    terms = list(terms)
    if combination not in COMBINATIONS:
        raise _unsupported(BAD_COMBINATION.format(combination=combination))
    for x in terms:
        if not isinstance(x, str) or not (x in WORDS or any(f in x for f in FAMILIES)):
            raise _unsupported(UNKNOWN_TERM.format(entry=x))
    ks = {f: _family_k(terms, f, n_base) for f in FAMILIES}
    if "visual" in terms and ks["VisualK"]:
        raise _unsupported(VISUAL_WITH_VISUALK)
    n = len(terms)
    return Plan(n_terms=n, weight=1.0 / n if n else 0.0, lingual="lingual" in terms, visual="visual" in terms, topk=ks["TopK"],
                wtopk=ks["WTopK"], lsda=ks["LSDA"], visualk=ks["VisualK"], average="Average" in terms, none="None" in terms,
                product=combination == "Product")


FINETUNE_WITH_REGRESSION_BRANCH = (
    "SupervisedDetectorOutputsFineTune with WEAK_DETECTOR.REGRESSION_BRANCH is not supported with these MODEL.ROI_HEADS.FINETUNE_TERMS (the shipped "
    "defaults hold \"visual\"): set FINETUNE_TERMS.CLASSIFIER, FINETUNE_TERMS.BBOX and FINETUNE_TERMS.MASK to [\"lingual\"] or []. ")


def check_regression_branch(plan, finetune=False):
    """with WEAK_DETECTOR.REGRESSION_BRANCH the reference's evaluation() returns no list of refinement streams: the per-RoI terms fail.
    finetune: the fine-tune ROI heads -- a fine-tune yaml that turns the switch on meets this refusal first, so it opens with the three lists to set"""
    from .inference import VISUAL_WITH_REGRESSION_BRANCH
    pre = FINETUNE_WITH_REGRESSION_BRANCH if finetune else ""
    if plan.visual:          # computed whenever any head lists it, under either combination (roi_heads.py:248)
        raise _unsupported(pre + VISUAL_WITH_REGRESSION_BRANCH)
    if plan.visualk and not plan.product:
        raise _unsupported(pre + VISUALK_WITH_REGRESSION_BRANCH)
