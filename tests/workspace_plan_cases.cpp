// Drives bayesml_amd/csrc/workspace_plan.h from a plain host compiler: tests/test_workspace_plan.py builds this file with
// -fsanitize=address,undefined, feeds it one case per line on stdin and compares what it prints.
//
//   options env.NAME=VALUE ...                                     -> WorkspaceOptions::read over that environment
//   shape   K= D= f64= max_rows= num_cu= ks.FIELD= ... env.NAME=   -> the WorkspaceShape, then one name:bytes:flags per buffer
//   life    (the same arguments)                                   -> creations over malloc with every allocation failing in
//                                                                     turn, alone and as a further tile; a group of three
//                                                                     destroyed in all six orders; a tile that is too large
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>

#include "../bayesml_amd/csrc/workspace_plan.h"

using namespace gmmvb;

namespace {

[[noreturn]] void die(const std::string& what) {
    std::fprintf(stderr, "%s\n", what.c_str());
    std::exit(2);
}
void expect(bool ok, const char* what) {
    if (!ok) die(std::string("life cycle: ") + what);
}

struct Case {
    std::map<std::string, std::string> env;
    std::map<std::string, int64_t> num;
    KernelSizes ks;
    WorkspaceOptions options() const {
        return WorkspaceOptions::read([this](const char* name) -> const char* {
            const auto it = env.find(name);
            return it == env.end() ? nullptr : it->second.c_str();
        });
    }
    WorkspaceShape shape(int64_t max_rows) const {
        return make_shape((int)num.at("K"), (int)num.at("D"), num.at("f64") ? GMMVB_F64 : GMMVB_F32, max_rows, (int)num.at("num_cu"),
                          options(), ks);
    }
    void set(const std::string& key, const std::string& val) {
        const int64_t v = std::atoll(val.c_str());
        if (key.compare(0, 4, "env.") == 0) env[key.substr(4)] = val;
        else if (key == "ks.max_tiles") ks.max_tiles = (int)v;
        else if (key == "ks.t1_splits") ks.t1_splits = (int)v;
        else if (key == "ks.sel_rows") ks.sel_rows = (int)v;
        else if (key == "ks.lse_rows") ks.lse_rows = (int)v;
        else if (key == "ks.scan_parts") ks.scan_parts = (int)v;
        else if (key == "ks.rec_slots") ks.rec_slots = (int)v;
        else if (key == "ks.mstep_components_per_wg") ks.mstep_components_per_wg = (int)v;
        else if (key == "ks.slab_len") ks.slab_len = (int)v;
        else if (key == "ks.estep_image_doubles") ks.estep_image_doubles = (int)v;
        else if (key == "ks.estep_tri_image_doubles") ks.estep_tri_image_doubles = (int)v;
        else if (key == "ks.estep_bound_blocks") ks.estep_bound_blocks = (int)v;
        else if (key == "ks.estep_i8_image_bytes") ks.estep_i8_image_bytes = (int)v;
        else if (key == "ks.estep_i8_bound_image_bytes") ks.estep_i8_bound_image_bytes = (int)v;
        else if (key == "ks.estep_i8_digit_row_bytes") ks.estep_i8_digit_row_bytes = v;
        else if (key == "ks.proj_image_len") ks.proj_image_len = v;
        else if (key == "ks.proj_const_len") ks.proj_const_len = v;
        else if (key == "ks.generic_rows") ks.generic_rows = (int)v;
        else num[key] = v;
    }
};

void print_options(const WorkspaceOptions& o) {
    std::printf("sparse=%d prune=%d variant_asked=%d sort_rows=%d settle_margin=%.17g opt_proof=%d opt_proof_all=%d opt_proof_blocked=%d "
                "opt_lazy=%d opt_project=%d opt_regroup_margin=%d gather_exit=%d cache_on=%d opt_carry_off=%d opt_hmm_mstep_dense=%d "
                "opt_calibrate=%d opt_debug=%d opt_mlist_xc=%d", (int)o.sparse, o.prune, o.variant_asked, (int)o.sort_rows, o.settle_margin,
                (int)o.opt_proof, (int)o.opt_proof_all, (int)o.opt_proof_blocked, (int)o.opt_lazy, o.opt_project,
                (int)o.opt_regroup_margin, (int)o.gather_exit, (int)o.cache_on, (int)o.opt_carry_off, (int)o.opt_hmm_mstep_dense,
                (int)o.opt_calibrate, (int)o.opt_debug, (int)o.opt_mlist_xc);
}

// ---- a workspace over malloc ---------------------------------------------------------------------------------------------
struct Malloc {
    int64_t gets = 0, fail_at = 0, live = 0;      // fail_at: the get of that number (1-based) fails; 0: none does
    std::set<void*> released;
    void* get(int64_t bytes, bool) {
        if (++gets == fail_at) return nullptr;
        ++live;
        return std::malloc((size_t)bytes);
    }
    bool zero(void* p, int64_t bytes, bool) {
        std::memset(p, 0, (size_t)bytes);
        return true;
    }
    void release(void* p, bool) {
        --live;
        released.insert(p);
        std::free(p);
    }
};
struct HostWorkspace {
    void* field[kBufCount] = {};
    void** at[kBufCount];
    BufferPlan plan;
    Scratch* group = nullptr;
    int64_t bytes = 0;
    HostWorkspace() {
        for (int i = 0; i < kBufCount; ++i) at[i] = &field[i];
    }
};
void destroy(HostWorkspace* ws, Malloc& a) {
    if (free_all(ws->plan, ws->at, ws->group, a)) delete ws->group;
    delete ws;
}
// the steps of create_workspace (capi.hip) that concern the buffers
HostWorkspace* create(const Case& c, int64_t max_rows, HostWorkspace* first, Malloc& a, const BufferSpec** failed = nullptr) {
    HostWorkspace* ws = new HostWorkspace();
    ws->group = first ? first->group : new Scratch();
    ++ws->group->refs;
    const WorkspaceShape s = c.shape(max_rows);
    if (!first) ws->group->npad = s.npad;
    ws->plan = buffer_plan(s, c.ks, ws->group->npad);
    const BufferSpec* f = allocate_all(ws->plan, ws->at, ws->group, a, &ws->bytes);
    if (failed) *failed = f;
    if (!f) return ws;
    destroy(ws, a);
    return nullptr;
}
// the group's buffers are still there to be written, from the first byte to the last (ASan would tell)
void touch_group(const Scratch* g) {
    for (int i = 0; i < kBufCount; ++i)
        if (g->buf[i]) static_cast<char*>(g->buf[i])[0] = static_cast<char*>(g->buf[i])[g->bytes[i] - 1] = 0x5a;
}

void life(const Case& c) {
    const int64_t rows = c.num.at("max_rows"), tile_rows = std::max<int64_t>(1, rows * 3 / 5);
    Malloc count;
    HostWorkspace* one = create(c, rows, nullptr, count);
    expect(one && one->bytes == one->plan.counted_bytes(), "bytes is the sum of the plan's counted sizes");
    const int64_t n_alloc = count.gets;
    expect(n_alloc == (int64_t)one->plan.size(), "one allocation per entry");
    destroy(one, count);
    expect(count.live == 0, "a destroyed workspace leaves nothing");
    for (int64_t n = 1; n <= n_alloc + 1; ++n) {       // the n-th allocation fails
        Malloc a;
        a.fail_at = n;
        HostWorkspace* ws = create(c, rows, nullptr, a);
        expect((ws == nullptr) == (n <= n_alloc), "creation fails exactly when an allocation does");
        if (ws) destroy(ws, a);
        expect(a.live == 0, "a failed creation leaves nothing");
    }
    int64_t n_tile = 0;
    if (!c.shape(rows).generic) {                      // (tile groups: non-generic workspaces only)
        {
            Malloc a;
            HostWorkspace* first = create(c, rows, nullptr, a);
            const int64_t before = a.gets;
            HostWorkspace* tile = create(c, tile_rows, first, a);
            expect(tile != nullptr, "a further tile");
            n_tile = a.gets - before;
            int64_t borrowed = 0;
            for (const BufferSpec& b : tile->plan) borrowed += (b.flags & kScratch) ? b.bytes : 0;
            expect(tile->bytes == tile->plan.counted_bytes() - borrowed, "a further tile does not count what it borrows");
            destroy(tile, a);
            destroy(first, a);
            expect(a.live == 0, "group of two");
        }
        for (int64_t n = 1; n <= n_tile + 1; ++n) {    // the n-th allocation of a further tile fails
            Malloc a;
            HostWorkspace* first = create(c, rows, nullptr, a);
            a.fail_at = a.gets + n;
            HostWorkspace* tile = create(c, tile_rows, first, a);
            expect((tile == nullptr) == (n <= n_tile), "the tile fails exactly when an allocation does");
            if (!tile) expect(first->group->refs == 1, "the failed tile gave its reference back");
            for (const BufferSpec& b : first->plan)
                if (b.flags & kScratch) expect(first->field[b.id] == first->group->buf[b.id] && !a.released.count(first->field[b.id]), "the first workspace's scratch is intact");
            touch_group(first->group);
            if (tile) destroy(tile, a);
            destroy(first, a);
            expect(a.live == 0, "a failed tile leaves nothing");
        }
        const int orders[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        for (const auto& order : orders) {             // a group of three: the scratch goes with the last reference
            Malloc a;
            HostWorkspace* w[3];
            w[0] = create(c, rows, nullptr, a);
            w[1] = create(c, tile_rows, w[0], a);
            w[2] = create(c, std::max<int64_t>(1, rows / 3), w[0], a);
            expect(w[1] && w[2] && w[0]->group->refs == 3, "three references");
            const Scratch* g = w[0]->group;
            void* const lnrho = g->buf[kBuf_lnrho];
            for (int i = 0; i < 3; ++i) {
                expect(!a.released.count(lnrho), "the scratch lives as long as a member does");
                touch_group(g);
                destroy(w[order[i]], a);
            }
            expect(a.released.count(lnrho) == 1 && a.live == 0, "the last reference frees the scratch, once");
        }
        {                                              // a tile larger than the first: refused before anything is allocated
            Malloc a;
            HostWorkspace* first = create(c, rows, nullptr, a);
            const int64_t gets = a.gets, live = a.live;
            const BufferSpec* failed = nullptr;
            HostWorkspace* tile = create(c, rows + 64, first, a, &failed);
            expect(!tile && failed && failed->code == GMMVB_EINVAL, "a larger tile is refused");
            expect(a.gets == gets && a.live == live && first->group->refs == 1, "... before anything is allocated for it");
            destroy(first, a);
            expect(a.live == 0, "after the refusal");
        }
    }
    std::printf("allocations=%lld tile_allocations=%lld ok=1\n", (long long)n_alloc, (long long)n_tile);
}

}  // namespace

int main() {
    for (std::string line; std::getline(std::cin, line);) {
        std::stringstream words(line);
        std::string kind;
        if (!(words >> kind) || kind[0] == '#') continue;
        Case c;
        for (std::string w; words >> w;) {
            const size_t eq = w.find('=');
            if (eq == std::string::npos) die("not key=value: '" + w + "'");
            c.set(w.substr(0, eq), w.substr(eq + 1));
        }
        if (kind == "options") {
            print_options(c.options());
            std::printf("\n");
        } else if (kind == "shape") {
            const WorkspaceShape s = c.shape(c.num.at("max_rows"));
            std::printf("T=%d wide=%d generic=%d npad=%lld KG=%d S_cap=%d split_rows=%lld img_len=%d variant=%d gen_S=%d lists=%d xc_len=%lld ",
                        s.T, (int)s.wide, (int)s.generic, (long long)s.npad, s.KG, s.S_cap, (long long)s.split_rows, s.img_len,
                        s.estep_variant, s.gen_S, (int)s.has_lists, (long long)s.xc_len);
            print_options(s);
            const BufferPlan p = buffer_plan(s, c.ks);
            std::printf(" counted_bytes=%lld |", (long long)p.counted_bytes());
            for (const BufferSpec& b : p) std::printf(" %s:%lld:%u", buffer_name(b.id), (long long)b.bytes, b.flags);
            std::printf("\n");
        } else if (kind == "life") {
            life(c);
        } else {
            die("unknown kind '" + kind + "'");
        }
    }
    return 0;
}
