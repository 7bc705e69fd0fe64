// Test driver of IndexIVF_HNSW::update_batch through the class surface (tests/test_gpu_upsert_class.py builds it with g++).
//   upsert_tool refused d nc code_size nsubc
//       an IndexIVF_HNSW_Grouping refuses update_batch: prints the message, exit status 0 when it threw.
//   upsert_tool search d nc code_size centroids info edges pq norm_pq opq|- in.index queries.fvecs nq k nprobe max_codes ef
//               new.fvecs labels.u32 update|pair out.bin out.index
//       search (the device copy is current from here on), then update_batch(new rows, labels) -- or, with pair, remove_ids(labels)
//       and add_batch(new rows, labels), the twin -- search, update_batch with one label repeated (update only: it must throw
//       std::invalid_argument and change nothing), search, invalidate_device(), search (the host lists uploaded again), write.
//       out.bin: labels [4][nq][k] (int64), distances [4][nq][k] (float), the removed count and "the repeat threw" (uint64 each).
// labels.u32 is a raw uint32 array, one label per row of new.fvecs.
#include <ivf-hnsw/IndexIVF_HNSW_Grouping.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ivfhnsw;
typedef IndexIVF_HNSW::idx_t idx_t;

static std::vector<idx_t> read_u32(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in)
        throw std::runtime_error(std::string("cannot open ") + path);
    in.seekg(0, std::ios::end);
    const size_t n = (size_t)in.tellg() / sizeof(uint32_t);
    in.seekg(0);
    std::vector<idx_t> v(n);
    in.read(reinterpret_cast<char *>(v.data()), n * sizeof(uint32_t));
    return v;
}

int main(int argc, char **argv)
try {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "refused" && argc == 6) {
        const size_t d = atol(argv[2]);
        IndexIVF_HNSW_Grouping index(d, atol(argv[3]), atol(argv[4]), 8, atol(argv[5]));
        std::vector<float> x(d, 0.f);
        const idx_t label = 7;
        try {
            index.update_batch(1, x.data(), &label);
        } catch (const std::runtime_error &e) {
            printf("refused: %s\n", e.what());
            return 0;
        }
        fprintf(stderr, "upsert_tool: a Grouping index took update_batch\n");
        return 1;
    }
    if (cmd != "search" || argc != 23)
        throw std::runtime_error("usage: see the head of upsert_tool.cpp");
    const size_t d = atol(argv[2]), nc = atol(argv[3]), cs = atol(argv[4]);
    const char *centroids = argv[5], *info = argv[6], *edges = argv[7], *ppq = argv[8], *pnorm = argv[9], *popq = argv[10],
               *pindex = argv[11], *pqueries = argv[12];
    const size_t nq = atol(argv[13]), k = atol(argv[14]), nprobe = atol(argv[15]), max_codes = atol(argv[16]), ef = atol(argv[17]);
    const char *pnew = argv[18];
    const std::vector<idx_t> labels = read_u32(argv[19]);
    const std::string mode = argv[20];
    if (mode != "update" && mode != "pair")
        throw std::runtime_error("mode must be update or pair");
    IndexIVF_HNSW *index = new IndexIVF_HNSW(d, nc, cs, 8);
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
    std::vector<float> q(nq * d), x(labels.size() * d);
    {
        std::ifstream in(pqueries, std::ios::binary);
        readXvec<float>(in, q.data(), d, nq);
        std::ifstream in2(pnew, std::ios::binary);
        readXvec<float>(in2, x.data(), d, labels.size());
    }
    std::vector<long> lab(4 * nq * k);
    std::vector<float> dist(4 * nq * k);
    uint64_t tail[2] = {0, 0};
    auto search = [&](size_t round) { index->search_batch(nq, k, q.data(), dist.data() + round * nq * k, lab.data() + round * nq * k); };
    search(0);
    if (mode == "update") {
        tail[0] = index->update_batch(labels.size(), x.data(), labels.data());
    } else {
        tail[0] = index->remove_ids(labels.size(), labels.data());
        index->add_batch(labels.size(), x.data(), labels.data());
    }
    search(1);
    if (mode == "update") {
        std::vector<idx_t> twice(labels);
        twice.back() = twice.front();
        try {
            index->update_batch(twice.size(), x.data(), twice.data());
        } catch (const std::invalid_argument &) {
            tail[1] = 1;
        }
    }
    search(2);
    index->invalidate_device();
    search(3);
    FILE *f = fopen(argv[21], "wb");
    if (!f)
        throw std::runtime_error("cannot write the result file");
    fwrite(lab.data(), sizeof(long), lab.size(), f);
    fwrite(dist.data(), sizeof(float), dist.size(), f);
    fwrite(tail, sizeof(uint64_t), 2, f);
    fclose(f);
    index->write(argv[22]);
    delete index;
    return 0;
} catch (const std::exception &e) {
    fprintf(stderr, "upsert_tool: %s\n", e.what());
    return 1;
}
