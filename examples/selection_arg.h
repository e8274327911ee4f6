// --selection puct|uct|improved of the example programs: the in-tree rule of Node::forward (policy.rs) as the TZ_SELECT_* value
// that tz_search_set_selection takes, -1 for an unknown name.
#pragma once
#include <string>

#include "takzero_hip.h"

static inline int selection_rule(const std::string& name) {
    return name == "puct" ? TZ_SELECT_PUCT : name == "uct" ? TZ_SELECT_UCT : name == "improved" ? TZ_SELECT_IMPROVED : -1;
}
