"""The reference's two hard-coded `instattn` rules (models/meta_basemodel.py:460-499) as AttentionRule objects.

The reference indexes the Alimama input matrix by column number: 5 = final_gender_code, 7 = pvalue_level, 8 = shopping_level,
15 = price (a DenseFeat column; as an attention field index 15 does not exist in a model whose 15 sparse fields are 0..14, so
the rules below name the fields and leave the choice of the price-like field to the caller).  Both rules use the threshold 0.2,
keep positives with pvalue_level == 3 only, and print a `classes_` lookup of the price that nothing in the reference sets - here
the input row is written out instead.

    model.flag = "sota-pos-showattn-instattn"
    model.instattn_rules = alimama_rules()
    model.predict(x_test, 4096, y_test)            # -> ./inst_attn_sota-pos-showattn-instattn.txt

or, without the flag:  model.attention_instances(x_test, y_test, rules=alimama_rules())
"""
from satrans_amd.attn_inst import AttentionRule

THRESHOLD = 0.2


def alimama_rules(price_field="brand", threshold=THRESHOLD):
    """`price_field`: the attention field that stands where the reference reads index 15 of the map (its own Alimama model
    carried the price as the 16th sparse field; with price as a DenseFeat, pick the field to look at)."""
    common = [("pvalue_level", "==", 3), ("pvalue_level", ">=", 2)]
    return [
        # :467  attn[7][5] > t and attn[7][15] > t and x[15] > 10000 and x[7] >= 2   (label 1, pvalue_level 3)
        AttentionRule([("pvalue_level", "final_gender_code", threshold), ("pvalue_level", price_field, threshold)],
                      label=1, where=common + [("price", ">", 10000)]),
        # :484  attn[15][7] > t and (attn[15][5] > t or attn[15][8] > t) and x[15] > 12000 and x[7] >= 2
        AttentionRule([(price_field, "pvalue_level", threshold),
                       [(price_field, "final_gender_code", threshold), (price_field, "shopping_level", threshold)]],
                      label=1, where=common + [("price", ">", 12000)]),
    ]
