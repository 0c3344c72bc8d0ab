// heap_order_check.cpp -- stand-alone program of tests/test_readcorrect_restated.py: the order in which
// std::priority_queue of this machine's standard library pops states that compare equivalent.  Reads operations from the
// standard input, "push <penalty> <pos> <id>" or "pop", and prints the id of every popped element ("-" when empty).
#include <cstdio>
#include <queue>
#include <vector>

struct state {
    int penalty, pos, id;
};
struct state_less {  // read_corrector.cpp:41-46
    bool operator()(const state &lhs, const state &rhs) const {
        return lhs.penalty < rhs.penalty || (lhs.penalty == rhs.penalty && lhs.pos < rhs.pos);
    }
};

int main() {
    std::priority_queue<state, std::vector<state>, state_less> q;
    char op[8];
    while (scanf("%7s", op) == 1) {
        if (op[1] == 'u') {
            state s;
            if (scanf("%d %d %d", &s.penalty, &s.pos, &s.id) != 3) return 2;
            q.emplace(s);
        } else if (q.empty()) {
            printf("-\n");
        } else {
            printf("%d\n", q.top().id);
            q.pop();
        }
    }
    return 0;
}
