// Test driver of the filter slots of the class surface (IndexIVF_HNSW::set_id_filter_slot, clear_id_filter_slot,
// search_batch_slots, range_search_slots; tests/test_gpu_filter_slots_class.py builds it with g++).  KIND is ivf
// (IndexIVF_HNSW) or grouping (IndexIVF_HNSW_Grouping).
//   filter_slots_tool KIND d nc code_size nsubc centroids info edges pq norm_pq opq|- in.index queries.fvecs nq k nprobe
//                     max_codes ef pruning query_slots.u8 nsets {slot deny labels.u32}... add.fvecs|- add_first_id
//                     clear_slot out.bin out.index
//       set_id_filter_slot of every set (no device copy yet: the first search installs them), round, add_batch(add rows,
//       ids add_first_id ..) when given, round, invalidate_device(), round, clear_id_filter_slot(clear_slot), round, write.
//       A round is search_batch_slots then range_search_slots at radius +inf.
//       out.bin, per round: labels [nq][k] (int64), distances [nq][k] (float), lims [nq + 1] (uint64), range labels
//       [lims[nq]] (int64), range distances [lims[nq]] (float).
// labels.u32 is a raw uint32 array, query_slots.u8 a raw byte array of nq entries.
#include <ivf-hnsw/IndexIVF_HNSW_Grouping.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ivfhnsw;

template <class T> static std::vector<T> read_raw(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in)
        throw std::runtime_error(std::string("cannot open ") + path);
    in.seekg(0, std::ios::end);
    const size_t n = (size_t)in.tellg() / sizeof(T);
    in.seekg(0);
    std::vector<T> v(n);
    in.read(reinterpret_cast<char *>(v.data()), n * sizeof(T));
    return v;
}

int main(int argc, char **argv)
try {
    if (argc < 22)
        throw std::runtime_error("usage: see the head of filter_slots_tool.cpp");
    const std::string kind = argv[1];
    const size_t d = atol(argv[2]), nc = atol(argv[3]), cs = atol(argv[4]), nsubc = atol(argv[5]);
    const char *centroids = argv[6], *info = argv[7], *edges = argv[8], *ppq = argv[9], *pnorm = argv[10], *popq = argv[11],
               *pindex = argv[12], *pqueries = argv[13];
    const size_t nq = atol(argv[14]), k = atol(argv[15]), nprobe = atol(argv[16]), max_codes = atol(argv[17]),
                 ef = atol(argv[18]);
    const bool pruning = atoi(argv[19]) != 0;
    const std::vector<uint8_t> qslots = read_raw<uint8_t>(argv[20]);
    if (qslots.size() != nq)
        throw std::runtime_error("query_slots.u8 must hold nq bytes");
    const int nsets = atoi(argv[21]);
    if (argc != 22 + 3 * nsets + 5)
        throw std::runtime_error("usage: see the head of filter_slots_tool.cpp");
    int a = 22 + 3 * nsets;
    const char *padd = argv[a];
    const IndexIVF_HNSW::idx_t add_first = (IndexIVF_HNSW::idx_t)atol(argv[a + 1]);
    const int clear_slot = atoi(argv[a + 2]);
    const char *pout = argv[a + 3], *pidx = argv[a + 4];
    IndexIVF_HNSW *index;
    if (kind == "grouping")
        index = new IndexIVF_HNSW_Grouping(d, nc, cs, 8, nsubc);
    else if (kind == "ivf")
        index = new IndexIVF_HNSW(d, nc, cs, 8);
    else
        throw std::runtime_error("KIND must be ivf or grouping");
    index->build_quantizer(centroids, info, edges, 16, 500);
    index->do_opq = strcmp(popq, "-") != 0;
    delete index->pq;
    index->pq = faiss::read_ProductQuantizer(ppq);
    if (index->do_opq)
        index->opq_matrix = dynamic_cast<faiss::LinearTransform *>(faiss::read_VectorTransform(popq));
    delete index->norm_pq;
    index->norm_pq = faiss::read_ProductQuantizer(pnorm);
    index->read(pindex);
    if (index->do_opq)
        index->rotate_quantizer();
    index->nprobe = nprobe;
    index->max_codes = max_codes;
    index->quantizer->efSearch = ef;
    if (auto *g = dynamic_cast<IndexIVF_HNSW_Grouping *>(index))
        g->do_pruning = pruning;
    std::vector<float> q(nq * d);
    {
        std::ifstream in(pqueries, std::ios::binary);
        readXvec<float>(in, q.data(), d, nq);
    }
    for (int s = 0; s < nsets; s++) {
        const std::vector<IndexIVF_HNSW::idx_t> lab = read_raw<IndexIVF_HNSW::idx_t>(argv[22 + 3 * s + 2]);
        index->set_id_filter_slot((unsigned)atoi(argv[22 + 3 * s]), lab.size(), lab.data(), atoi(argv[22 + 3 * s + 1]) != 0);
    }
    FILE *f = fopen(pout, "wb");
    if (!f)
        throw std::runtime_error("cannot write the result file");
    auto round = [&]() {
        std::vector<long> lab(nq * k);
        std::vector<float> dist(nq * k);
        index->search_batch_slots(nq, k, q.data(), qslots.data(), dist.data(), lab.data());
        fwrite(lab.data(), sizeof(long), lab.size(), f);
        fwrite(dist.data(), sizeof(float), dist.size(), f);
        std::vector<size_t> lims;
        std::vector<long> rl;
        std::vector<float> rd;
        index->range_search_slots(nq, q.data(), qslots.data(), INFINITY, lims, rd, rl);
        fwrite(lims.data(), sizeof(size_t), lims.size(), f);
        fwrite(rl.data(), sizeof(long), rl.size(), f);
        fwrite(rd.data(), sizeof(float), rd.size(), f);
    };
    round();
    if (strcmp(padd, "-") != 0) {
        std::ifstream bin(padd, std::ios::binary);
        bin.seekg(0, std::ios::end);
        const size_t nb = (size_t)bin.tellg() / (sizeof(int) + d * sizeof(float));
        bin.seekg(0);
        std::vector<float> base(nb * d);
        readXvec<float>(bin, base.data(), d, nb);
        std::vector<IndexIVF_HNSW::idx_t> ids(nb);
        for (size_t i = 0; i < nb; i++)
            ids[i] = add_first + (IndexIVF_HNSW::idx_t)i;
        index->add_batch(nb, base.data(), ids.data());
    }
    round();
    index->invalidate_device(); // the next search uploads everything again, the slots with it
    round();
    index->clear_id_filter_slot(clear_slot);
    round();
    fclose(f);
    index->write(pidx);
    delete index;
    return 0;
} catch (const std::exception &e) {
    fprintf(stderr, "filter_slots_tool: %s\n", e.what());
    return 1;
}
