// tests/cpp/dense_split_rule_check.cpp -- align_rules.h db3_plan, printed for tests/test_dense_split_host.py: the program of
// dense_bf16_rule_check.cpp (same arguments, same output line) asking the split kernel's rule instead of the bf16 kernel's.
#include "align_rules.h"
#define db16_plan db3_plan
#include "dense_bf16_rule_check.cpp"
